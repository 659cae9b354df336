"""f64 statement of Config.DUAL_RMSPROP on the vector-state network (GAME = 'Pendulum-v0') for the tests (not collected: no
test_ prefix).  DESIGN.md 8h; the rules are 8c's, restated for this net's 16 variables.

Reference NetworkVP.py:107-147: cost_p = -(cost_p_1_agg + cost_p_2_agg) and cost_v each get an RMSProp optimizer with the
same hyperparameters, both stepped by one train call on one forward pass.  TF-1 drops a variable whose gradient is None, so
the value optimizer has no slot for logits_p/out_x/*, logits_p/out_y/* and the policy optimizer none for logits_v/* (cost_p
sees v only through tf.stop_gradient, :99); the trunk gets both steps.  With USE_GRAD_CLIP every gradient tensor of both
costs is clipped on its own by tf.clip_by_norm (:128-138).  The network applies the value step, then the policy step; in f64
the order does not matter.

Built from mlp_oracle's forward and the dv / dz of its loss_and_grads, which it does not modify, and like them it follows the
dtype of the weights: float32 weights give the float32 restatement that tests/closeness.py's bound is measured with.
"""
import numpy as np

import mlp_oracle as m

HEAD_P = ("logits_p/out_x/w", "logits_p/out_x/b", "logits_p/out_y/w", "logits_p/out_y/b")
HEAD_V = ("logits_v/w", "logits_v/b")
TRUNK_VARS = tuple(k for k in m.PARAM_ORDER if k not in HEAD_P + HEAD_V)
DELTAS = ("dd1", "dpd4", "dpd3", "dpd2", "dpd1")


def _stream(params, f, dv, dhx, dhy):
    """The backward recursion of mlp_oracle.loss_and_grads from the head deltas (dv [B], dhx [B,A], dhy [B,A]) -> dict of
    the 16 gradients and the five trunk deltas."""
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
    for l in range(len(m.TRUNK) - 1, -1, -1):
        name = m.TRUNK[l][0]
        g[dnames[l]] = delta
        g[name + "/w"] = ins[l].T @ delta
        g[name + "/b"] = delta.sum(axis=0)
        if l > 0:
            delta = delta @ params[name + "/w"].T
            if m.TRUNK[l - 1][2]:
                delta = delta * outs[l - 1] * (1.0 - outs[l - 1])
    return g


def dual_grads(params, x, y_r, a, beta, adv_const=None):
    """(losses, g_p, g_v): the gradients of cost_p and of cost_v, each keyed like params plus the per-row deltas 'dv', 'dz',
    'dd1', 'dpd4' ... 'dpd1' of that cost: the recursion run once from (0, dz) and once from (dv, 0).  Exact zeros where a
    cost has no path (g_p on logits_v/*, g_v on logits_p/*, and the other cost's head delta)."""
    losses, g = m.loss_and_grads(params, x, y_r, a, beta, adv_const=adv_const)
    f = m.forward(params, x)
    A = params["logits_p/out_x/b"].shape[0]
    dv, dz = g["dv"], g["dz"]
    dhx, dhy = dz[:, :A], dz[:, A:]
    gp = _stream(params, f, np.zeros_like(dv), dhx, dhy)
    gv = _stream(params, f, dv, np.zeros_like(dhx), np.zeros_like(dhy))
    gp.update(dv=np.zeros_like(dv), dz=dz)
    gv.update(dv=dv, dz=np.zeros_like(dz))
    return losses, gp, gv


def clip_by_norm(g, clip):
    """tf.clip_by_norm (NetworkVP.py:128-138): g * clip / max(||g||_2, clip)."""
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
    for k in m.PARAM_ORDER:
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


def norms(g):
    """{variable: ||g||_2} of one cost's gradients."""
    return {k: float(np.sqrt(np.sum(np.asarray(g[k], np.float64) ** 2))) for k in m.PARAM_ORDER}


def region_mask(state_dim, num_actions, names):
    """Boolean mask over the flat arena: True on the variables in `names`."""
    shapes = m.param_shapes(state_dim, num_actions)
    return np.concatenate([np.full(int(np.prod(shapes[k])), k in names) for k in m.PARAM_ORDER])
