"""f64 statement of Config.CONTINUOUS_INPUT for the tests (not collected: no test_ prefix).

Reference NetworkVP.py:92,95-105,175-204: the policy output is the angle of two sigmoid dense heads of the hidden layer,
    X = sigmoid(d1 Wx + bx) - 0.5, Y = sigmoid(d1 Wy + by) - 0.5, o = atan2(Y, X) / pi   (in (-1, 1])
and softmax_p = log_softmax_p = o, so
    cost_p_1 = (sum_k o_k a_k) (y_r - stop_gradient(v)), cost_p_2 = -beta sum_k o_k o_k, cost_p = -(sum cost_p_1 + sum cost_p_2)
with cost_v, the optimizer and clipping as on the discrete path.  The gradient is TF-1's: Atan2Grad divided by pi, then the
sigmoids.  Nothing guards X = Y = 0 (NaN there, as in TF); the tests keep away from it and from the branch cut X < 0, Y = 0.

The trunk is oracle.ga3c_oracle's (its _conv_fwd / _conv_bwd, which this file does not modify).
"""
import numpy as np

import ga3c_oracle as o

PARAM_ORDER = o.PARAM_ORDER[:8] + ("logits_p/out_x/w", "logits_p/out_x/b", "logits_p/out_y/w", "logits_p/out_y/b")
HEADS = PARAM_ORDER[8:]
INIT = 0.3                              # U(-0.3, 0.3) for the heads' weights and biases (NetworkVP.py:194-204)


def param_shapes(num_actions):
    s = {k: v for k, v in o.param_shapes(num_actions).items() if not k.startswith("logits_p/")}
    for xy in ("x", "y"):
        s["logits_p/out_%s/w" % xy] = (o.HID, num_actions)
        s["logits_p/out_%s/b" % xy] = (num_actions,)
    return s


def init_params(num_actions, seed=12345):
    """The trunk and logits_v of oracle.init_params; the two heads U(-0.3, 0.3) from PCG64(seed + 1)."""
    p = {k: v for k, v in o.init_params(num_actions, seed).items() if not k.startswith("logits_p/")}
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    shapes = param_shapes(num_actions)
    for k in HEADS:
        p[k] = rng.uniform(-INIT, INIT, size=shapes[k]).astype(np.float32).astype(np.float64)
    return p


def _sigmoid(h):
    return 1.0 / (1.0 + np.exp(-h))


def forward(params, x, keep=False):
    """-> dict(o [B,A], v [B], z [B,2A] = [hx | hy]) (+ activations with keep)."""
    x = np.asarray(x)
    bsz = x.shape[0]
    x = x.reshape(bsz, o.H, o.W, o.C)
    n1pre, cols1 = o._conv_fwd(x, params["conv11/w"], params["conv11/b"], o.CONV1)
    n1 = np.maximum(n1pre, 0)
    n2pre, cols2 = o._conv_fwd(n1, params["conv12/w"], params["conv12/b"], o.CONV2)
    n2 = np.maximum(n2pre, 0)
    flat = n2.reshape(bsz, o.FLAT)
    d1pre = flat @ params["dense1/w"] + params["dense1/b"]
    d1 = np.maximum(d1pre, 0)
    v = (d1 @ params["logits_v/w"] + params["logits_v/b"])[:, 0]
    hx = d1 @ params["logits_p/out_x/w"] + params["logits_p/out_x/b"]
    hy = d1 @ params["logits_p/out_y/w"] + params["logits_p/out_y/b"]
    sx, sy = _sigmoid(hx), _sigmoid(hy)
    X, Y = sx - 0.5, sy - 0.5
    out = dict(o=np.arctan2(Y, X) / np.pi, v=v, z=np.concatenate([hx, hy], axis=1))
    if keep:
        out.update(cols1=cols1, n1=n1, cols2=cols2, n2=n2, flat=flat, d1=d1, sx=sx, sy=sy, X=X, Y=Y,
                   n1pre=n1pre, n2pre=n2pre, d1pre=d1pre)
    return out


def loss_and_grads(params, x, y_r, a, beta, adv_const=None, relu_on=None, f=None):
    """(losses, grads): losses = dict(cost_p_1_agg, cost_p_2_agg, cost_v, cost_all); grads keyed like params plus 'dz'
    ([B,2A] = [dhx | dhy]), 'dv', 'dd1', 'dn2', 'dn1'.  adv_const freezes y_r - v for finite differences (tf.stop_gradient).
    The dtype follows x / params (y_r and a are cast to it), so that a float32 run stays float32 throughout; relu_on is
    oracle.loss_and_grads' (the units through which the backward pass flows, default: those with a positive output)."""
    f = forward(params, x, keep=True) if f is None else f       # f: the caller's forward(params, x, keep=True)
    dt = f["z"].dtype
    y_r, a = np.asarray(y_r).astype(dt), np.asarray(a).astype(dt)
    beta = dt.type(beta)
    out, v = f["o"], f["v"]
    adv = y_r - v if adv_const is None else np.asarray(adv_const).astype(dt)
    cost_p_1 = (out * a).sum(axis=1) * adv
    cost_p_2 = -beta * (out * out).sum(axis=1)
    g_o = -a * adv[:, None] + 2.0 * beta * out                 # d cost_p / d o
    X, Y = f["X"], f["Y"]
    r2 = X * X + Y * Y
    dX = -Y * g_o / (np.pi * r2)                                # Atan2Grad, then the division by pi
    dY = X * g_o / (np.pi * r2)
    dhx = dX * f["sx"] * (1.0 - f["sx"])
    dhy = dY * f["sy"] * (1.0 - f["sy"])
    dv = v - y_r
    c1, c2 = cost_p_1.sum(), cost_p_2.sum()
    cost_v = 0.5 * np.sum((y_r - v) ** 2)
    losses = dict(cost_p_1_agg=c1, cost_p_2_agg=c2, cost_v=cost_v, cost_all=-(c1 + c2) + cost_v)

    d1, flat, n2, n1 = f["d1"], f["flat"], f["n2"], f["n1"]
    on = {k: np.asarray(relu_on[k]).reshape(f[k].shape) if relu_on is not None else f[k] > 0 for k in ("d1", "n2", "n1")}
    g = {}
    g["logits_p/out_x/w"] = d1.T @ dhx
    g["logits_p/out_x/b"] = dhx.sum(axis=0)
    g["logits_p/out_y/w"] = d1.T @ dhy
    g["logits_p/out_y/b"] = dhy.sum(axis=0)
    g["logits_v/w"] = d1.T @ dv[:, None]
    g["logits_v/b"] = dv.sum(keepdims=True)
    dd1 = (dhx @ params["logits_p/out_x/w"].T + dhy @ params["logits_p/out_y/w"].T +
           dv[:, None] @ params["logits_v/w"].T) * on["d1"]
    g["dense1/w"] = flat.T @ dd1
    g["dense1/b"] = dd1.sum(axis=0)
    dn2 = (dd1 @ params["dense1/w"].T).reshape(n2.shape) * on["n2"]
    g["conv12/w"], g["conv12/b"], dn1 = o._conv_bwd(dn2, f["cols2"], params["conv12/w"], o.CONV2, 21, True)
    dn1 = dn1 * on["n1"]
    g["conv11/w"], g["conv11/b"], _ = o._conv_bwd(dn1, f["cols1"], params["conv11/w"], o.CONV1, 84, False)
    g["dz"], g["dv"], g["dd1"], g["dn2"], g["dn1"] = np.concatenate([dhx, dhy], axis=1), dv, dd1, dn2, dn1
    return losses, g


def rmsprop_update(params, ms, grads, lr, decay=0.99, eps=0.1, momentum=0.0, mom=None, clip=None):
    """TF-1.x ApplyRMSProp over the 12 variables, in place; clip: tf.clip_by_average_norm per variable first."""
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


def unflat(theta, num_actions):
    shapes, out, off = param_shapes(num_actions), {}, 0
    for k in PARAM_ORDER:
        n = int(np.prod(shapes[k]))
        out[k] = np.asarray(theta[off:off + n], np.float64).reshape(shapes[k])
        off += n
    return out


def safe_rows(params, x, min_abs_y=1e-4, f=None):
    """Rows of x whose every action keeps away from the branch cut (X < 0, |Y| < min_abs_y) and from X = Y = 0.
    f: forward(params, x, keep=True) where the caller has it already."""
    f = forward(params, x, keep=True) if f is None else f
    bad = ((f["X"] < 0) & (np.abs(f["Y"]) < min_abs_y)) | (np.hypot(f["X"], f["Y"]) < min_abs_y)
    return ~bad.any(axis=1)
