"""f64 statement of Config.DUAL_RMSPROP for the tests (not collected: no test_ prefix).

NetworkVP_discrate.py:87-99,108-117,126-127: cost_p = -(cost_p_1_agg + cost_p_2_agg) and cost_v each get an RMSProp
optimizer with the same hyperparameters, both stepped by one train call on one forward pass.  TF-1 drops a variable whose
gradient is None, so the value optimizer has no slot for logits_p/* and the policy optimizer none for logits_v/* (cost_p sees
v only through tf.stop_gradient, :78); the trunk gets both steps.  With USE_GRAD_CLIP every gradient tensor of both costs
is clipped on its own by tf.clip_by_norm.  The engine applies the value step, then the policy step;
in f64 the order does not matter.

Built from oracle.ga3c_oracle's own pieces (forward, loss_and_grads for dz / dv, _conv_bwd), which it does not modify.
"""
import numpy as np

import ga3c_oracle as o

HEAD_P = ("logits_p/w", "logits_p/b")
HEAD_V = ("logits_v/w", "logits_v/b")


def _trunk(params, f, dd1, g, on):
    """The trunk's gradient for the upstream gradient dd1 of the hidden layer (the lines of loss_and_grads, per cost)."""
    g["dense1/w"] = f["flat"].T @ dd1
    g["dense1/b"] = dd1.sum(axis=0)
    dn2 = (dd1 @ params["dense1/w"].T).reshape(f["n2"].shape) * on["n2"]
    g["conv12/w"], g["conv12/b"], dn1 = o._conv_bwd(dn2, f["cols2"], params["conv12/w"], o.CONV2, 21, True)
    dn1 = dn1 * on["n1"]
    g["conv11/w"], g["conv11/b"], _ = o._conv_bwd(dn1, f["cols1"], params["conv11/w"], o.CONV1, 84, False)
    g["dd1"], g["dn2"], g["dn1"] = dd1, dn2, dn1


def dual_grads(params, x, y_r, a, beta, log_eps=1e-6, min_policy=0.0, use_log_softmax=False, relu_on=None, f=None):
    """(losses, g_p, g_v): the gradients of cost_p and of cost_v, each keyed like params (zeros where a cost has no path),
    plus each cost's own 'dd1', 'dn2', 'dn1' and the head deltas 'dz' (g_p) and 'dv' (g_v).  The dtype follows x / params;
    relu_on is oracle.loss_and_grads' (the units through which both backward passes flow)."""
    if f is None:       # (f: the caller's forward(params, x, min_policy, use_log_softmax, keep=True); one pass serves both calls)
        f = o.forward(params, x, min_policy, use_log_softmax, keep=True)
    losses, g = o.loss_and_grads(params, x, y_r, a, beta, log_eps=log_eps, min_policy=min_policy,
                                 use_log_softmax=use_log_softmax, relu_on=relu_on, f=f)
    on = {k: np.asarray(relu_on[k]).reshape(f[k].shape) if relu_on is not None else f[k] > 0 for k in ("d1", "n2", "n1")}
    d1, dz, dv = f["d1"], g["dz"], g["dv"]
    gp = {k: np.zeros_like(params[k]) for k in HEAD_V}
    gv = {k: np.zeros_like(params[k]) for k in HEAD_P}
    gp["logits_p/w"] = d1.T @ dz
    gp["logits_p/b"] = dz.sum(axis=0)
    gv["logits_v/w"] = d1.T @ dv[:, None]
    gv["logits_v/b"] = dv.sum(keepdims=True)
    _trunk(params, f, (dz @ params["logits_p/w"].T) * on["d1"], gp, on)
    _trunk(params, f, (dv[:, None] @ params["logits_v/w"].T) * on["d1"], gv, on)
    gp["dz"], gv["dv"] = dz, dv
    return losses, gp, gv


def clip_by_norm(g, clip):
    """tf.clip_by_norm (NetworkVP_discrate.py:108-117): g * clip / max(||g||_2, clip)."""
    return g * clip / max(np.sqrt(np.sum(g * g)), clip)


def init_slots(params):
    """Both optimizers' slots over the whole arena (ms = 1, mom = 0); regions without a slot keep these values."""
    return {"ms_p": {k: np.ones_like(t) for k, t in params.items()},
            "mom_p": {k: np.zeros_like(t) for k, t in params.items()},
            "ms_v": {k: np.ones_like(t) for k, t in params.items()},
            "mom_v": {k: np.zeros_like(t) for k, t in params.items()}}


def _rms(g, ms, mom, k, lr, decay, eps, momentum):
    ms[k] = decay * ms[k] + (1.0 - decay) * g * g
    step = lr * g / np.sqrt(ms[k] + eps)
    if momentum != 0.0:
        mom[k] = momentum * mom[k] + step
        step = mom[k]
    return step


def dual_rmsprop_update(params, slots, gp, gv, lr, decay=0.99, eps=0.1, momentum=0.0, clip=None):
    """Both optimizers' steps (TF-1.x ApplyRMSProp each), in place; a head is stepped only by its own cost's optimizer."""
    for k in o.PARAM_ORDER:
        step = np.zeros_like(params[k])
        if k not in HEAD_P:
            g = np.asarray(gv[k]).reshape(params[k].shape)
            if clip is not None:
                g = clip_by_norm(g, clip)
            step = step + _rms(g, slots["ms_v"], slots["mom_v"], k, lr, decay, eps, momentum)
        if k not in HEAD_V:
            g = np.asarray(gp[k]).reshape(params[k].shape)
            if clip is not None:
                g = clip_by_norm(g, clip)
            step = step + _rms(g, slots["ms_p"], slots["mom_p"], k, lr, decay, eps, momentum)
        params[k] = params[k] - step
    return params


def flat(d):
    return np.concatenate([np.asarray(d[k]).reshape(-1) for k in o.PARAM_ORDER])


def region_mask(num_actions, names):
    """Boolean mask over the flat arena: True on the variables in `names`."""
    shapes = o.param_shapes(num_actions)
    return np.concatenate([np.full(int(np.prod(shapes[k])), k in names) for k in o.PARAM_ORDER])
