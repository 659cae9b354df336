"""f64 statement of the DDPG handle's soft actor-critic step (Config.DDPG_SOFT, ga3c_ddpg_soft_create) for the tests
(not collected: no test_ prefix): Haarnoja et al. 2018 on top of tests/ddpg_oracle.py and tests/td3_oracle.py.  The handle is a
twin handle whose actor_output/W is [300, 2A] and which has one more variable, actor_soft/log_alpha [1].

Head and sample.  o = a2 W_o + b_o (ddpg_oracle.actor_forward's "ho", 2A wide); mu = o[:, :A]; ls = clip(o[:, A:], ls_min, ls_max);
no gradient reaches o[:, A + i] unless ls_min < o < ls_max; sigma = exp(ls); u = mu + sigma eps; a = tanh(u);
    logp = sum_i (((-eps_i^2 / 2 - ls_i) - ln sqrt(2 pi)) - log1mtanh2(u_i)),  i ascending,
    log1mtanh2(u) = ln(1 - tanh^2 u) = 2 ((ln 2 - |u|) - log1p(exp(-2 |u|))), from u: tanh rounds to 1 from |u| = 9 (f32) on.
Draws.  normal(seed, stream, j) is td3_oracle's Box-Muller on device_agents_oracle.uniform, (f32), unclipped.  With t = step + 1,
row k and action i, j = k A + i: the target's eps2 is stream 2 t, the policy step's eps stream 2 t + 1, both of `seed`.  A
prediction's row r draws j = c A + i of stream r under seed + 1 at the handle's prediction count c.
Step, with alpha = exp(log_alpha) as it stands before the step:
  1. a2, logp2 = the ONLINE actor's sample at s2 under eps2.  q' = min of both target critics at (s2, a2); v' = q' - alpha logp2;
     y = r on a done row or without `future`, else r + g v' (g: gamma, or the row's discount).
  2. td3_oracle's step of both critics on y (paired form, importance weights, clip_by_norm, RMSProp or Adam at count t).
  3. Only when t % policy_delay == 0, against the updated critics: a, logp = the sample at s under eps; q1, q2 there; per row the
     smaller selects its critic, critic 1 on a tie; g = dq_sel/da; J = (1/B) sum_k (alpha logp_k - q_sel,k), a MEAN over the rows;
     du = (2 alpha a - g dtanh(u)) / B, dmu = du, dls = du sigma eps - alpha / B inside the clamp, else 0; the actor's Adam at
     count t / policy_delay; then log_alpha's Adam at alpha_lr x lr and the same count on the gradient of
     -log_alpha (mean_k logp_k + target_entropy), the mean summed in row order; the soft update of all three nets.
As in ddpg_oracle every function follows the dtype of the weights it is given.
"""
import numpy as np

import ddpg_oracle as o
import device_agents_oracle as da
import td3_oracle as t3

LOG_ALPHA = "actor_soft/log_alpha"
ALL_VARS = t3.ALL_VARS + (LOG_ALPHA,)                 # the engine's order: the twin's 38, then the temperature
TRAINABLE = t3.TRAINABLE + (LOG_ALPHA,)
LN2, HALF_LN_2PI = float(np.log(2.0)), float(0.5 * np.log(2.0 * np.pi))


def shapes(S, A):
    sh = t3.shapes(S, A)
    sh.update({"actor_output/W": (o.H2, 2 * A), "actor_output/b": (2 * A,), LOG_ALPHA: (1,)})
    return sh


def random_params(S, A, rng, scale=0.3, stats=False, log_alpha=np.log(0.2)):
    """td3_oracle.random_params' 38, then the Gaussian head by the same rule over its wider shape, drawn after them."""
    p = t3.random_params(S, A, rng, scale, stats)
    for k in ("actor_output/W", "actor_output/b"):
        p[k] = rng.uniform(-scale, scale, shapes(S, A)[k]).astype(np.float32).astype(np.float64)
    p[LOG_ALPHA] = np.array([log_alpha], np.float32).astype(np.float64)
    return p


def normal(seed, stream, j):
    """8n's Box-Muller draw j (array) of `stream` (scalar or array) -> float32, unclipped."""
    j = np.asarray(j, np.uint64)
    u1 = 1.0 - da.uniform(seed, stream, 2 * j)
    u2 = da.uniform(seed, stream, 2 * j + 1)
    return (np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)).astype(np.float32)


def step_draws(seed, t, B, A):
    """-> (eps2, eps) [B, A] float32 of step t: streams 2 t and 2 t + 1."""
    j = np.arange(B * A, dtype=np.uint64)
    return normal(seed, 2 * t, j).reshape(B, A), normal(seed, 2 * t + 1, j).reshape(B, A)


def predict_draws(seed, c, B, A):
    """eps [B, A] float32 of the prediction at count c: row r is stream r of seed + 1, draw c A + i."""
    out = np.empty((B, A), np.float32)
    for r in range(B):
        out[r] = normal(seed + 1, r, c * A + np.arange(A, dtype=np.uint64))
    return out


def log1mtanh2(u):
    au = np.abs(u)
    return 2.0 * ((LN2 - au) - np.log1p(np.exp(-2.0 * au)))


def head(P, s, ls_min, ls_max):
    """-> dict: ddpg_oracle.actor_forward's trunk, raw = o [B, 2A], mu, ls (clamped), inside (bool: the clamp passes a gradient)."""
    f = o.actor_forward(P, s)
    A = f["ho"].shape[1] // 2
    raw = f["ho"]
    lo = raw[:, A:]
    f.update(raw=raw, mu=raw[:, :A], ls=np.clip(lo, ls_min, ls_max), inside=(lo > ls_min) & (lo < ls_max))
    return f


def logp_of(eps, ls, u):
    """The log-density of a = tanh(u), u = mu + exp(ls) eps, summed in i order."""
    terms = ((-0.5 * eps * eps - ls) - HALF_LN_2PI) - log1mtanh2(u)
    s = np.zeros(terms.shape[0], terms.dtype)
    for i in range(terms.shape[1]):
        s = s + terms[:, i]
    return s


def sample(P, s, eps, ls_min=-20.0, ls_max=2.0):
    """-> head()'s dict + eps, sigma, u, a, logp."""
    f = head(P, s, ls_min, ls_max)
    eps = np.asarray(eps, f["mu"].dtype)
    sigma = np.exp(f["ls"])
    u = f["mu"] + sigma * eps
    f.update(eps=eps, sigma=sigma, u=u, a=np.tanh(u), logp=logp_of(eps, f["ls"], u))
    return f


def mean_action(P, s, ls_min=-20.0, ls_max=2.0):
    return np.tanh(head(P, s, ls_min, ls_max)["mu"])


def targets(O, T, s2, r, done, gamma, eps2, future=True, ls_min=-20.0, ls_max=2.0):
    """Step 1 -> dict(y, qt = min q', qt1, qt2, a2, logp2, vt); gamma: a scalar or the rows' discounts."""
    r = np.asarray(r, T["critic_fc1/W"].dtype)
    if not future:
        return dict(y=r.copy(), qt=None, qt1=None, qt2=None, a2=None, logp2=None, vt=None, eps2=np.asarray(eps2))
    f = sample(O, s2, eps2, ls_min, ls_max)
    qt1 = o.critic_forward(T, s2, f["a"])["q"][:, 0]
    qt2 = o.critic_forward(t3.critic2(T), s2, f["a"])["q"][:, 0]
    qt = np.minimum(qt1, qt2)
    vt = qt - np.exp(O[LOG_ALPHA][0]) * f["logp"]
    y = np.where(np.asarray(done) != 0, r, r + np.asarray(gamma, r.dtype) * vt)
    return dict(y=y, qt=qt, qt1=qt1, qt2=qt2, a2=f["a"], logp2=f["logp"], vt=vt, eps2=np.asarray(eps2), fwd2=f)


def policy_grads(O, s, eps, target_entropy, ls_min=-20.0, ls_max=2.0):
    """Step 3's gradients against the critics as O holds them -> dict(fwd, pq1, pq2, sel (True: critic 2), g, g1, g2, do [B, 2A],
    actor_grads, mean_logp, dlog_alpha, J)."""
    f = sample(O, s, eps, ls_min, ls_max)
    B, A = f["a"].shape
    alpha = np.exp(O[LOG_ALPHA][0])
    O2 = t3.critic2(O)
    q1 = o.critic_forward(O, s, f["a"])["q"][:, 0]
    q2 = o.critic_forward(O2, s, f["a"])["q"][:, 0]
    g1, g2 = o.action_gradient(O, s, f["a"]), o.action_gradient(O2, s, f["a"])
    sel = q2 < q1                                        # critic 1 on a tie
    g = np.where(sel[:, None], g2, g1)
    du = (2.0 * alpha * f["a"] - g * o.dtanh(f["u"])) / B
    dls = np.where(f["inside"], du * f["sigma"] * f["eps"] - alpha / B, 0.0)
    do = np.concatenate([du, dls], axis=1)
    G = {"actor_output/W": f["a2"].T @ do, "actor_output/b": do.sum(0)}
    dn2 = (do @ O["actor_output/W"].T) * (f["n2"] > 0)
    G["actor_norm2/beta"] = dn2.sum(0)
    G["actor_norm2/gamma"] = (dn2 * f["xh2"]).sum(0)
    dh2 = dn2 * (O["actor_norm2/gamma"] * f["rs2"])
    G["actor_fc2/W"] = f["a1"].T @ dh2
    G["actor_fc2/b"] = dh2.sum(0)
    dn1 = (dh2 @ O["actor_fc2/W"].T) * (f["n1"] > 0)
    G["actor_norm1/beta"] = dn1.sum(0)
    G["actor_norm1/gamma"] = (dn1 * f["xh1"]).sum(0)
    dh1 = dn1 * (O["actor_norm1/gamma"] * f["rs1"])
    G["actor_fc1/W"] = f["x"].T @ dh1
    G["actor_fc1/b"] = dh1.sum(0)
    f.update(do=do, dn2=dn2, dn1=dn1)
    total = f["logp"].dtype.type(0.0)
    for k in range(B):                                   # the mean's order: rows ascending
        total = total + f["logp"][k]
    mean_logp = total / B
    q_sel = np.where(sel, q2, q1)
    return dict(fwd=f, pq1=q1, pq2=q2, sel=sel, g=g, g1=g1, g2=g2, do=do, actor_grads=G, mean_logp=mean_logp,
                dlog_alpha=-(mean_logp + target_entropy), J=float(np.mean(alpha * f["logp"] - q_sel)))


def relu_margin(O, T, s, a, s2, eps2, ls_min=-20.0, ls_max=2.0):
    """Per row: the smallest |pre-activation| of any relu unit in the evaluations every soft step makes: the online actor at s2,
    both target critics at (s2, a2), both online critics at (s, a)."""
    f2 = sample(O, s2, eps2, ls_min, ls_max)
    fs = [(f2, ("n1", "n2")), (o.critic_forward(T, s2, f2["a"]), ("n1", "t")), (o.critic_forward(t3.critic2(T), s2, f2["a"]), ("n1", "t")),
          (o.critic_forward(O, s, a), ("n1", "t")), (o.critic_forward(t3.critic2(O), s, a), ("n1", "t"))]
    return np.min([np.abs(f[k]).min(axis=1) for f, ks in fs for k in ks], axis=0)


def policy_margin(O, s, eps, ls_min=-20.0, ls_max=2.0):
    """Per row, for the policy step against the critics as O holds them: (the smallest |pre-activation| of any relu unit of the
    actor at s and of both critics at (s, a), |q1 - q2| / max(1, |q1|, |q2|))."""
    f = sample(O, s, eps, ls_min, ls_max)
    c1, c2 = o.critic_forward(O, s, f["a"]), o.critic_forward(t3.critic2(O), s, f["a"])
    fs = [(f, ("n1", "n2")), (c1, ("n1", "t")), (c2, ("n1", "t"))]
    q1, q2 = c1["q"][:, 0], c2["q"][:, 0]
    gap = np.abs(q1 - q2) / np.maximum(1.0, np.maximum(np.abs(q1), np.abs(q2)))
    return np.min([np.abs(g[k]).min(axis=1) for g, ks in fs for k in ks], axis=0), gap


def new_state(online, target, critic_rmsprop=True):
    """td3_oracle.new_state over the 31 trainable variables; log_alpha's slots are Adam's."""
    st = dict(online={k: v.copy() for k, v in online.items()}, target={k: v.copy() for k, v in target.items()},
              slot_a={}, slot_b={}, step=0)
    for k in TRAINABLE:
        rms = critic_rmsprop and k not in o.ACTOR_TRAINABLE and k != LOG_ALPHA
        st["slot_a"][k] = np.ones_like(online[k]) if rms else np.zeros_like(online[k])
        st["slot_b"][k] = np.zeros_like(online[k])
    return st


def train_step(st, s, a, r, done, s2, lr, *, policy_delay=2, seed=0, eps2=None, eps=None, per_w=None, disc=None, alpha_lr=1.0,
               target_entropy=None, ls_min=-20.0, ls_max=2.0, actor_lr=1.0, critic_lr=10.0, tau=0.001, gamma=0.99, future=True,
               critic_rmsprop=True, decay=0.99, momentum=0.0, rms_eps=0.1, clip=None, stop_after=6):
    """One soft step on `st` in place.  eps2 / eps: the draws [B, A] if given (the device's, fetched), else drawn.  per_w:
    importance weights or None.  disc: the rows' discounts or None (gamma).  -> dict; stop_after as td3_oracle.train_step's."""
    O, T = st["online"], st["target"]
    t = st["step"] + 1
    policy = t % policy_delay == 0
    B, A = np.shape(a)
    if target_entropy is None:
        target_entropy = -float(A)
    d2, d1 = step_draws(seed, t, B, A)
    eps2 = d2 if eps2 is None else eps2
    eps = d1 if eps is None else eps
    out = targets(O, T, s2, r, done, gamma if disc is None else disc, eps2, future, ls_min, ls_max)
    out["policy"] = policy
    y = out["y"]
    for tag, P, pre in (("", O, "critic_"), ("2", t3.critic2(O), "critic2_")):
        f, dq, g = o.critic_grads(P, s, a, y, "paired") if per_w is None else t3._weighted(P, s, a, y, per_w)
        out["q" + tag], out["dq" + tag], out["critic%s_grads" % tag], out["critic%s_fwd" % tag] = f["q"][:, 0].copy(), dq, g, f
        for k in o.CRITIC_TRAINABLE:
            if k == o.DEAD:
                continue
            gk = o.clip_by_norm(g[k], clip) if clip else g[k]
            name = pre + k[len("critic_"):]
            if critic_rmsprop:
                o.rmsprop_step(P[k], st["slot_a"][name], st["slot_b"][name], gk, critic_lr * lr, decay, momentum, rms_eps)
            else:
                o.adam_step(P[k], st["slot_a"][name], st["slot_b"][name], gk, critic_lr * lr, t)
    out["q_max"], out["q_avg"] = float(out["q"].max()), float(out["q"].mean())
    if stop_after <= 3 or (not policy and stop_after <= 4):
        return out
    if policy:
        pg = policy_grads(O, s, eps, target_entropy, ls_min, ls_max)
        out.update(pg, eps=np.asarray(eps))
        if stop_after <= 4:
            return out
        for k in o.ACTOR_TRAINABLE:
            o.adam_step(O[k], st["slot_a"][k], st["slot_b"][k], pg["actor_grads"][k].reshape(O[k].shape), actor_lr * lr, t // policy_delay)
        o.adam_step(O[LOG_ALPHA], st["slot_a"][LOG_ALPHA], st["slot_b"][LOG_ALPHA], np.array([pg["dlog_alpha"]]), alpha_lr * lr,
                    t // policy_delay)
        for k in t3.TRAINABLE:                           # (log_alpha's target copy is not touched)
            T[k] = tau * O[k] + (1.0 - tau) * T[k]
    st["step"] = t
    return out
