"""The parameters and batches of the vector-state network's GPU tests, and the cases of tests/test_vector_limits_cpu.py and
tests/test_gpu_vector_limits.py (not collected: no test_ prefix): ga3c_mlp at the limits of the shapes ga3c_mlp_create admits
(state_dim 1 .. 64, num_actions 1 .. 32) and with a saturated angle head.  Both files build their cases here, so the conditions
the CPU file asserts are the conditions of the rows the GPU file runs.

    params(S, A), batch(params, B, S, A, seed)     what tests/test_gpu_vector_net.py has always used (it imports them)
    SHAPES x SIZES                                 NH = 1 + 2A = 3, 65, 65, 3, 35, 63 head columns; batch seed 100 + B
    saturated_params(S, A)                         both angle heads' weights x 100: sigmoids at exactly 0 and 1 in float32

    close, config, reset, mask, e32               the small helpers the GPU files of this network share

No case or condition here touches a kernel; a condition is the float64 oracle's statement about the rows."""
import contextlib
import functools

import numpy as np

import closeness as c
import mlp_oracle as m

TOL = 1e-4

SHAPES = [(1, 1), (64, 32), (1, 32), (64, 1), (33, 17), (5, 31)]
SIZES = [1, 15, 16, 17, 132]          # the tile is 16 rows: one row, a tile short by one, full, plus one, 8 tiles + 4
MAX_BATCH = 160
BETA = 0.01
MIN_KEPT = 0.90                       # share of the candidate rows that safe_rows must keep

SATURATED = [(7, 3), (64, 32)]
SAT_SCALE = 100.0
SAT_B, SAT_SEED = 132, 21
ONE, OVERFLOW, LINEAR = 17.0, 88.8, 2.0   # |h| from which the f32 sigmoid is exactly 1; where expf(-h) overflows; the mild range
MIN_ONE, MIN_LINEAR = 0.25, 0.02      # shares of the saturated logits beyond ONE and inside LINEAR


def params(state_dim, num_actions):
    p = m.init_params(state_dim, num_actions, seed=777)
    rng = np.random.default_rng(5)
    p["logits_p/out_x/b"] = rng.uniform(-1.5, 1.5, num_actions).astype(np.float32).astype(np.float64)
    p["logits_p/out_y/b"] = rng.uniform(-1.5, 1.5, num_actions).astype(np.float32).astype(np.float64)
    return p


def _draw(params, bsz, state_dim, num_actions, seed):
    """-> (candidate rows, which of them safe_rows keeps, a, y) from one PCG64(seed) stream."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.uniform(-1.5, 1.5, size=(3 * bsz + 16, state_dim)).astype(np.float32)
    keep = m.safe_rows(params, x.astype(np.float64), 1e-3)
    a = rng.uniform(-1, 1, size=(bsz, num_actions)).astype(np.float32)
    y = rng.uniform(-1, 1, size=bsz).astype(np.float32)
    return x, keep, a, y


def batch(params, bsz, state_dim, num_actions, seed):
    x, keep, a, y = _draw(params, bsz, state_dim, num_actions, seed)
    x = x[keep][:bsz]
    assert x.shape[0] == bsz
    return x, y, a


def close(got, want, tol=TOL):
    """The project's rule: max|got - want| <= tol x max(1, max|want|)."""
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    return np.max(np.abs(got - want)) <= tol * max(1.0, np.max(np.abs(want)))


@contextlib.contextmanager
def config(**kw):
    """Config with the given settings for the length of the block."""
    import ga3c_amd  # noqa: F401
    from Config import Config
    saved = {k: getattr(Config, k) for k in kw}
    for k, v in kw.items():
        setattr(Config, k, v)
    try:
        yield Config
    finally:
        for k, v in saved.items():
            setattr(Config, k, v)


def reset(net, params, dual=True):
    """theta = params, ms = 1, mom = 0 (both optimizers' slots when there are two)."""
    net.set_arena(0, m.flat(params))
    for w in (1, 4) if dual else (1,):
        net.set_arena(w, np.ones(net.param_count, np.float32))
    for w in (2, 5) if dual else (2,):
        net.set_arena(w, np.zeros(net.param_count, np.float32))


def mask(net, names):
    """Boolean mask over the handle's flat arena: True on the variables in `names`."""
    out = np.zeros(net.param_count, bool)
    for k in names:
        off, size = net._offsets[k]
        out[off:off + size] = True
    return out


def e32(name, got32, want64, head32, head64, num_actions):
    """closeness's e32 of one tensor: the oracle in float32 against the oracle in float64; a bias gradient of ONE element
    takes the larger of that single draw and what the float32 error of the delta it sums implies (closeness.e32_of_row_sum;
    head32 / head64 hold that delta, 'dv' and 'dz')."""
    e = c.rel_err(got32[name], want64[name])
    sums = {"logits_v/b": ("dv", slice(None)), "logits_p/out_x/b": ("dz", (slice(None), slice(0, num_actions))),
            "logits_p/out_y/b": ("dz", (slice(None), slice(num_actions, 2 * num_actions)))}
    if name in sums and np.size(want64[name]) == 1:
        key, sel = sums[name]
        e = max(e, c.e32_of_row_sum(np.asarray(head32[key])[sel], np.asarray(head64[key])[sel]))
    return e


def rows_kept(params, bsz, state_dim, num_actions, seed):
    """-> (candidate rows that safe_rows keeps, candidate rows) of batch(...)'s draw."""
    _, keep, _, _ = _draw(params, bsz, state_dim, num_actions, seed)
    return int(keep.sum()), int(keep.size)


@functools.lru_cache(maxsize=None)
def limit_params(state_dim, num_actions):
    """params(S, A), built once per shape; the tests copy before they step it."""
    return params(state_dim, num_actions)


@functools.lru_cache(maxsize=None)
def limit_batch(state_dim, num_actions, bsz):
    return batch(limit_params(state_dim, num_actions), bsz, state_dim, num_actions, 100 + bsz)


@functools.lru_cache(maxsize=None)
def saturated_params(state_dim, num_actions):
    """init_params(seed = 777) with both angle heads' weights x 100, rounded through float32 as every test weight is."""
    p = m.init_params(state_dim, num_actions, seed=777)
    for k in ("logits_p/out_x/w", "logits_p/out_y/w"):
        p[k] = (p[k] * SAT_SCALE).astype(np.float32).astype(np.float64)
    return p


@functools.lru_cache(maxsize=None)
def saturated_batch(state_dim, num_actions, seed=SAT_SEED, bsz=SAT_B):
    return batch(saturated_params(state_dim, num_actions), bsz, state_dim, num_actions, seed)


def f64(*arrays):
    return [np.asarray(t, np.float64) for t in arrays]


def f32_params(p):
    return {k: np.asarray(v, np.float32) for k, v in p.items()}


def saturation(z):
    """-> dict(max, one, overflow, linear): max |z|, the share of logits beyond ONE, how many are beyond OVERFLOW, the share
    inside LINEAR."""
    az = np.abs(np.asarray(z, np.float64))
    return dict(max=float(az.max()), one=float(np.mean(az > ONE)), overflow=int(np.sum(az > OVERFLOW)),
                linear=float(np.mean(az < LINEAR)))


def check_kept(state_dim, num_actions, bsz, p=None, seed=None):
    """The rows-kept condition of one (shape, size) -> (kept, candidates)."""
    p = limit_params(state_dim, num_actions) if p is None else p
    kept, total = rows_kept(p, bsz, state_dim, num_actions, 100 + bsz if seed is None else seed)
    assert kept >= MIN_KEPT * total, (state_dim, num_actions, bsz, kept, total)
    return kept, total


def check_saturated(state_dim, num_actions):
    """The conditions on a saturated case, from the float64 oracle -> (saturation(z), (kept, candidates))."""
    p = saturated_params(state_dim, num_actions)
    x, _, _ = saturated_batch(state_dim, num_actions)
    s = saturation(m.forward(p, x.astype(np.float64))["z"])
    assert s["one"] >= MIN_ONE and s["overflow"] >= 1 and s["linear"] >= MIN_LINEAR, (state_dim, num_actions, s)
    return s, check_kept(state_dim, num_actions, SAT_B, p, SAT_SEED)


def no_zero_tensor(tensors, names, where):
    """closeness.rel_err refuses an all-zero reference: none of the compared tensors of the oracle is one."""
    for k in names:
        assert np.any(tensors[k]), (where, k)
