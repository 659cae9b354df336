"""f64 statement of the vector-state network for the tests (not collected: no test_ prefix).  forward / loss_and_grads
follow the dtype of the weights: float64 is the statement, float32 weights give the like-for-like restatement that
tests/closeness.py's bound is measured with.

Reference NetworkVP.py:67-105,175-210 (GAME = 'Pendulum-v0'): dense_layer = x W + b with U(-0.3, 0.3) weights and biases,
    pd1 = x W11 + b11, pd2 = pd1 W12 + b12, pd3 = pd2 W13 + b13, pd4 = sigmoid(pd3 W14 + b14), d1 = sigmoid(pd4 W1 + b1)
    v = d1 Wv + bv;  the angle head of tests/continuous_oracle.py on d1 (X = sigmoid(hx) - 0.5, Y = sigmoid(hy) - 0.5,
    o = atan2(Y, X) / pi), its policy cost and TF-1 gradient, cost_v, RMSProp and clip_by_average_norm as there.
"""
import numpy as np

import ga3c_oracle as o

TRUNK = (("dense11_p", 4, False), ("dense12_p", 256, False), ("dense13_p", 256, False), ("dense14_p", 100, True),
         ("dense1", 64, True))
HEADS = ("logits_v", "logits_p/out_x", "logits_p/out_y")
PARAM_ORDER = tuple("%s/%s" % (n, wb) for n in [t[0] for t in TRUNK] + list(HEADS) for wb in ("w", "b"))
INIT = 0.3


def param_shapes(state_dim, num_actions):
    s, fan = {}, state_dim
    for name, width, _ in TRUNK:
        s[name + "/w"], s[name + "/b"] = (fan, width), (width,)
        fan = width
    for name, width in zip(HEADS, (1, num_actions, num_actions)):
        s[name + "/w"], s[name + "/b"] = (fan, width), (width,)
    return s


def param_count(state_dim, num_actions):
    return 4 * state_dim + 99305 + 130 * num_actions


def init_params(state_dim, num_actions, seed=12345):
    """U(-0.3, 0.3) from one PCG64(seed) stream in variable order, f32-rounded (what NetworkVP_vector.initial_arena draws)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    shapes = param_shapes(state_dim, num_actions)
    return {k: rng.uniform(-INIT, INIT, size=shapes[k]).astype(np.float32).astype(np.float64) for k in PARAM_ORDER}


def _sigmoid(h):
    return 1.0 / (1.0 + np.exp(-h))


def forward(params, x):
    """-> dict(o [B,A], v [B], z [B,2A] = [hx | hy], pd1..pd4, d1, and the head intermediates)."""
    dt = params["dense1/w"].dtype
    h = np.asarray(x, dt)
    out = {"x": h}
    keys = ("pd1", "pd2", "pd3", "pd4", "d1")
    for (name, _, sig), key in zip(TRUNK, keys):
        h = h @ params[name + "/w"] + params[name + "/b"]
        if sig:
            h = _sigmoid(h)
        out[key] = h
    d1 = h
    v = (d1 @ params["logits_v/w"] + params["logits_v/b"])[:, 0]
    hx = d1 @ params["logits_p/out_x/w"] + params["logits_p/out_x/b"]
    hy = d1 @ params["logits_p/out_y/w"] + params["logits_p/out_y/b"]
    sx, sy = _sigmoid(hx), _sigmoid(hy)
    X, Y = sx - dt.type(0.5), sy - dt.type(0.5)
    out.update(o=np.arctan2(Y, X) / dt.type(np.pi), v=v, z=np.concatenate([hx, hy], axis=1), sx=sx, sy=sy, X=X, Y=Y)
    return out


def loss_and_grads(params, x, y_r, a, beta, adv_const=None):
    """(losses, grads): losses = dict(cost_p_1_agg, cost_p_2_agg, cost_v, cost_all); grads keyed like params plus the
    per-row deltas at every pre-activation: 'dv', 'dz' [B,2A], 'dd1', 'dpd4', 'dpd3', 'dpd2', 'dpd1'.
    adv_const freezes y_r - v for finite differences (tf.stop_gradient)."""
    f = forward(params, x)
    dt = f["v"].dtype
    y_r, a = np.asarray(y_r, dt), np.asarray(a, dt)
    out, v = f["o"], f["v"]
    adv = y_r - v if adv_const is None else np.asarray(adv_const, dt)
    cost_p_1 = (out * a).sum(axis=1) * adv
    cost_p_2 = -beta * (out * out).sum(axis=1)
    g_o = -a * adv[:, None] + 2.0 * beta * out
    X, Y = f["X"], f["Y"]
    r2 = X * X + Y * Y
    pi = dt.type(np.pi)
    dhx = (-Y * g_o / (pi * r2)) * f["sx"] * (1.0 - f["sx"])
    dhy = (X * g_o / (pi * r2)) * f["sy"] * (1.0 - f["sy"])
    dv = v - y_r
    c1, c2 = cost_p_1.sum(), cost_p_2.sum()
    cost_v = 0.5 * np.sum((y_r - v) ** 2)
    losses = dict(cost_p_1_agg=c1, cost_p_2_agg=c2, cost_v=cost_v, cost_all=-(c1 + c2) + cost_v)

    g = {}
    d1 = f["d1"]
    for name, dl in (("logits_v", dv[:, None]), ("logits_p/out_x", dhx), ("logits_p/out_y", dhy)):
        g[name + "/w"] = d1.T @ dl
        g[name + "/b"] = dl.sum(axis=0)
    delta = (dv[:, None] @ params["logits_v/w"].T + dhx @ params["logits_p/out_x/w"].T +
             dhy @ params["logits_p/out_y/w"].T) * d1 * (1.0 - d1)
    ins = (f["x"], f["pd1"], f["pd2"], f["pd3"], f["pd4"])
    outs = (f["pd1"], f["pd2"], f["pd3"], f["pd4"], f["d1"])
    dnames = ("dpd1", "dpd2", "dpd3", "dpd4", "dd1")
    for l in range(len(TRUNK) - 1, -1, -1):
        name, _, _ = TRUNK[l]
        g[dnames[l]] = delta
        g[name + "/w"] = ins[l].T @ delta
        g[name + "/b"] = delta.sum(axis=0)
        if l > 0:
            delta = delta @ params[name + "/w"].T
            if TRUNK[l - 1][2]:
                delta = delta * outs[l - 1] * (1.0 - outs[l - 1])
    g["dz"], g["dv"] = np.concatenate([dhx, dhy], axis=1), dv
    return losses, g


def rmsprop_update(params, ms, grads, lr, decay=0.99, eps=0.1, momentum=0.0, mom=None, clip=None):
    """TF-1.x ApplyRMSProp over the 16 variables, in place; clip: tf.clip_by_average_norm per variable first."""
    for k in PARAM_ORDER:
        g = np.asarray(grads[k]).reshape(params[k].shape)
        if clip is not None:
            g = o.clip_by_average_norm(g, clip)
        ms[k] = decay * ms[k] + (1.0 - decay) * g * g
        step = lr * g / np.sqrt(ms[k] + eps)
        if momentum != 0.0:
            mom[k] = momentum * mom[k] + step
            step = mom[k]
        params[k] = params[k] - step
    return params, ms


def flat(d):
    return np.concatenate([np.asarray(d[k]).reshape(-1) for k in PARAM_ORDER])


def unflat(theta, state_dim, num_actions):
    shapes, out, off = param_shapes(state_dim, num_actions), {}, 0
    for k in PARAM_ORDER:
        n = int(np.prod(shapes[k]))
        out[k] = np.asarray(theta[off:off + n], np.float64).reshape(shapes[k])
        off += n
    return out


def safe_rows(params, x, min_abs_y=1e-4):
    """Rows of x whose every action keeps away from the atan2 branch cut and from X = Y = 0."""
    f = forward(params, x)
    bad = ((f["X"] < 0) & (np.abs(f["Y"]) < min_abs_y)) | (np.hypot(f["X"], f["Y"]) < min_abs_y)
    return ~bad.any(axis=1)
