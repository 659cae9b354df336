"""f64 statement of the discrete-action vector-state network for the tests (not collected: no test_ prefix).  forward /
loss_and_grads follow the dtype of the weights: float64 is the statement; handed float32 weights and rows they compute in
float32 throughout, which is the like-for-like restatement that tests/closeness.py's bound is measured with.

Reference NetworkVP_discrate.py:39-130, NetworkVP.py:194-210 (GAME = 'CartPole-v0'): dense_layer = sigmoid(x W + b) with
U(-0.3, 0.3) weights and biases;
    stack 'fork'    h_i = sigmoid(x W_i + b_i) for every i, all of them from x; the heads read h_L; layers 1..L-1 are dead
    stack 'chained' h_i = sigmoid(h_{i-1} W_i + b_i), h_0 = x
    v = h_L Wv + bv;  z = h_L Wp + bp;  softmax, loss and head gradients: the lines of oracle/ga3c_oracle.py (:61-85,100 of
    the reference), RMSProp and clip_by_average_norm as there.  A dead variable has gradient exactly 0 and is skipped by the
    optimizer: value, ms and mom stay as they are.
"""
import numpy as np

import ga3c_oracle as o

HEADS = ("logits_v", "logits_p")
INIT = 0.3
DEFAULT_LAYERS = (10, 10, 10, 10)


def layer_names(layers):
    return tuple("dense1_%d_p" % (i + 1) for i in range(len(layers)))


def param_order(layers=DEFAULT_LAYERS):
    return tuple("%s/%s" % (n, wb) for n in layer_names(layers) + HEADS for wb in ("w", "b"))


def param_shapes(state_dim, num_actions, layers=DEFAULT_LAYERS, stack="fork"):
    s, fan = {}, state_dim
    for name, width in zip(layer_names(layers), layers):
        s[name + "/w"], s[name + "/b"] = (fan, width), (width,)
        if stack == "chained":
            fan = width
    for name, width in zip(HEADS, (1, num_actions)):
        s[name + "/w"], s[name + "/b"] = (layers[-1], width), (width,)
    return s


def param_count(state_dim, num_actions, layers=DEFAULT_LAYERS, stack="fork"):
    return sum(int(np.prod(v)) for v in param_shapes(state_dim, num_actions, layers, stack).values())


def dead_params(layers=DEFAULT_LAYERS, stack="fork"):
    if stack == "chained":
        return ()
    return tuple("%s/%s" % (n, wb) for n in layer_names(layers)[:-1] for wb in ("w", "b"))


def init_params(state_dim, num_actions, layers=DEFAULT_LAYERS, stack="fork", seed=12345):
    """U(-0.3, 0.3) from one PCG64(seed) stream in variable order, f32-rounded (what NetworkVP_discrate.initial_arena draws)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    shapes = param_shapes(state_dim, num_actions, layers, stack)
    return {k: rng.uniform(-INIT, INIT, size=shapes[k]).astype(np.float32).astype(np.float64) for k in param_order(layers)}


def _sigmoid(h):
    return 1.0 / (1.0 + np.exp(-h))


def _nlayers(params):
    return (len(params) - 4) // 2


def forward(params, x, stack="fork", min_policy=0.0, use_log_softmax=False):
    """-> dict(p [B,A], v [B], z [B,A], s (the plain softmax), x, h1..hL (live layers only), zs, e)."""
    dt = params["logits_v/w"].dtype
    x = np.asarray(x, dt)
    nl = _nlayers(params)
    out = {"x": x}
    h = x
    for i in range(nl):
        if stack == "fork" and i < nl - 1:
            continue
        name = "dense1_%d_p" % (i + 1)
        h = _sigmoid((h if stack == "chained" else x) @ params[name + "/w"] + params[name + "/b"])
        out["h%d" % (i + 1)] = h
    v = (h @ params["logits_v/w"] + params["logits_v/b"])[:, 0]
    z = h @ params["logits_p/w"] + params["logits_p/b"]
    zs = z - z.max(axis=1, keepdims=True)
    e = np.exp(zs)
    s = e / e.sum(axis=1, keepdims=True)
    num_actions = z.shape[1]
    p = s if use_log_softmax else (s + dt.type(min_policy)) / (dt.type(1.0) + dt.type(min_policy) * dt.type(num_actions))
    out.update(p=p, v=v, z=z, s=s, zs=zs, e=e)
    return out


def loss_and_grads(params, x, y_r, a, beta, stack="fork", log_eps=1e-6, min_policy=0.0, use_log_softmax=False, adv_const=None):
    """(losses, grads): losses = dict(cost_p_1_agg, cost_p_2_agg, cost_v, cost_all); grads keyed like params (exact zeros for
    the dead variables) plus the per-row deltas at every live pre-activation: 'dv', 'dz', 'dh<i>'.
    adv_const freezes y_r - v for finite differences (tf.stop_gradient)."""
    f = forward(params, x, stack, min_policy, use_log_softmax)
    dt = f["z"].dtype
    beta, log_eps, min_policy = dt.type(beta), dt.type(log_eps), dt.type(min_policy)
    y_r, a = np.asarray(y_r, dt), np.asarray(a, dt)
    z, p, v, s = f["z"], f["p"], f["v"], f["s"]
    num_actions = z.shape[1]
    adv = y_r - v if adv_const is None else np.asarray(adv_const, dt)
    if use_log_softmax:
        ls = f["zs"] - np.log(f["e"].sum(axis=1, keepdims=True))
        lsel = (ls * a).sum(axis=1)
        cost_p_1 = lsel * adv
        cost_p_2 = -beta * (ls * s).sum(axis=1)
        ent = (s * ls).sum(axis=1, keepdims=True)
        dz = -adv[:, None] * (a - s * a.sum(axis=1, keepdims=True)) + beta * s * (ls - ent)
    else:
        sel = (p * a).sum(axis=1)
        cost_p_1 = np.log(np.maximum(sel, log_eps)) * adv
        logp = np.log(np.maximum(p, log_eps))
        cost_p_2 = -beta * (logp * p).sum(axis=1)
        one, zero = dt.type(1.0), dt.type(0.0)
        g_sel = np.where(sel >= log_eps, one / np.maximum(sel, log_eps), zero)      # tf.maximum routes the gradient to x >= eps
        g_p = -(adv * g_sel)[:, None] * a + beta * (logp + np.where(p >= log_eps, one, zero))
        g_s = g_p / (one + min_policy * dt.type(num_actions))
        dz = s * (g_s - (g_s * s).sum(axis=1, keepdims=True))
    dv = v - y_r
    cost_v = dt.type(0.5) * np.sum((y_r - v) ** 2)
    c1, c2 = cost_p_1.sum(), cost_p_2.sum()
    losses = dict(cost_p_1_agg=c1, cost_p_2_agg=c2, cost_v=cost_v, cost_all=-(c1 + c2) + cost_v)

    nl = _nlayers(params)
    g = {k: np.zeros_like(val) for k, val in params.items()}
    hl = f["h%d" % nl]
    g["logits_v/w"], g["logits_v/b"] = hl.T @ dv[:, None], dv.sum(keepdims=True)
    g["logits_p/w"], g["logits_p/b"] = hl.T @ dz, dz.sum(axis=0)
    delta = (dv[:, None] @ params["logits_v/w"].T + dz @ params["logits_p/w"].T) * hl * (1.0 - hl)
    for i in range(nl, 0, -1):
        name = "dense1_%d_p" % i
        src = f["h%d" % (i - 1)] if (stack == "chained" and i > 1) else f["x"]
        g["dh%d" % i] = delta
        g[name + "/w"], g[name + "/b"] = src.T @ delta, delta.sum(axis=0)
        if stack != "chained" or i == 1:
            break
        hp = f["h%d" % (i - 1)]
        delta = (delta @ params[name + "/w"].T) * hp * (1.0 - hp)
    g["dz"], g["dv"] = dz, dv
    return losses, g


def rmsprop_update(params, ms, grads, lr, stack="fork", decay=0.99, eps=0.1, momentum=0.0, mom=None, clip=None):
    """TF-1.x ApplyRMSProp over the live variables, in place; clip: tf.clip_by_average_norm per variable first.  Dead
    variables are skipped: value, ms and mom untouched."""
    nl = _nlayers(params)
    layers = tuple(params["dense1_%d_p/b" % (i + 1)].shape[0] for i in range(nl))
    dead = dead_params(layers, stack)
    for k in param_order(layers):
        if k in dead:
            continue
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


def train_step(params, ms, mom, x, y_r, a, lr, beta, stack="fork", momentum=0.0, clip=None, decay=0.99, eps=0.1, **kw):
    losses, g = loss_and_grads(params, x, y_r, a, beta, stack=stack, **kw)
    rmsprop_update(params, ms, g, lr, stack=stack, decay=decay, eps=eps, momentum=momentum, mom=mom, clip=clip)
    return losses, g


def flat(d):
    nl = _nlayers(d)
    layers = tuple(d["dense1_%d_p/b" % (i + 1)].shape[0] for i in range(nl))
    return np.concatenate([np.asarray(d[k]).reshape(-1) for k in param_order(layers)])
