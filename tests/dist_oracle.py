"""f64 statement of the DDPG handle's distributional step (ga3c_ddpg_dist_create, Config.DDPG_DISTRIBUTIONAL) for
the tests (not collected: no test_ prefix).  Built on ddpg_oracle's networks, backward pass and optimizers, as td3_oracle is.

The critic predicts a categorical distribution over N fixed returns and is trained by cross-entropy against the projected
target distribution (Bellemare et al. 2017, "C51"); the actor ascends its expectation (Barth-Maron et al. 2018, "D4PG").

    support   z_k = vmin + k delta, delta = (vmax - vmin) / (N - 1), from the f32-rounded vmin and vmax the handle is given
    head      critic_output/W [300,N], /b [N]; logits = c2 W + b; p = softmax(logits), the row maximum subtracted first;
              q = sum_k z_k p_k
    target    p' = softmax of the target critic at (s2, actor_target(s2)); g_i = 0 on a done row or without `future`, else the
              row's discount (a scalar gamma or one per row); Tz_j = clip(r_i + g_i z_j, vmin, vmax); b_j = (Tz_j - vmin) / delta;
              m_k = sum_j p'_j max(0, 1 - |b_j - k|)  -- the projection in gather form (project);  y = sum z m, qt = sum z p'.
              Without `future` no target net is evaluated: p' and qt are zero and m_k = max(0, 1 - |b - k|), b from r alone.
    critic    L = (1/B) sum_i w_i ce_i, ce_i = -sum_k m_ik log p_ik; dz_ik = (w_i / B)(p_ik - m_ik); the delta at the second
              layer is relu'(t) (dz W^T); below that ddpg_oracle.critic_grads' backward pass
    actor     dQ/dlogit_k = p_k (z_k - Q) of the updated critic at (s, actor(s) + noise); g = dQ/da from it

Every function follows the dtype of the weights it is given, as ddpg_oracle's do.
"""
import numpy as np

import ddpg_oracle as o

ACTOR_TRAINABLE, CRITIC_TRAINABLE, TRAINABLE, ALL_VARS, DEAD = o.ACTOR_TRAINABLE, o.CRITIC_TRAINABLE, o.TRAINABLE, o.ALL_VARS, o.DEAD
new_state = o.new_state


def shapes(S, A, N):
    sh = o.shapes(S, A)
    sh.update({"critic_output/W": (o.H2, N), "critic_output/b": (N,)})
    return sh


def random_params(S, A, N, rng, scale=0.3, stats=False):
    """ddpg_oracle.random_params with the head at [300,N], [N]: drawn after the others, so that those are what they are there."""
    p = o.random_params(S, A, rng, scale, stats)
    for k in ("critic_output/W", "critic_output/b"):
        p[k] = rng.uniform(-scale, scale, shapes(S, A, N)[k]).astype(np.float32).astype(np.float64)
    return p


def support(N, vmin, vmax, dtype=np.float64):
    """-> (z [N], vmin, vmax, delta) in `dtype`, from the f32-rounded ends."""
    lo, hi = dtype(np.float32(vmin)), dtype(np.float32(vmax))
    delta = (hi - lo) / dtype(N - 1)
    return lo + np.arange(N, dtype=dtype) * delta, lo, hi, delta


def softmax(logits):
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def log_softmax(logits):
    t = logits - logits.max(axis=1, keepdims=True)
    return t - np.log(np.exp(t).sum(axis=1, keepdims=True))


def head(P, x, a):
    """-> ddpg_oracle.critic_forward's dict, its "q" being the logits [B,N], + p [B,N]."""
    f = o.critic_forward(P, x, a)
    f["p"] = softmax(f["q"])
    return f


def project(pt, r, g, N, vmin, vmax):
    """m [B,N] = the projection of the distribution pt [B,N] on r_i + g_i z onto the support, in gather form:
    m_ik = sum_j pt_ij max(0, 1 - |b_ij - k|).  pt None: all the mass at r_i (g is not read)."""
    dtype = np.float64 if pt is None else pt.dtype.type
    z, lo, hi, delta = support(N, vmin, vmax, dtype)
    r = np.asarray(r, dtype)
    k = np.arange(N, dtype=dtype)
    if pt is None:
        b = (np.clip(r, lo, hi) - lo) / delta
        return np.maximum(0.0, 1.0 - np.abs(b[:, None] - k[None, :]))
    b = (np.clip(r[:, None] + np.asarray(g, dtype)[:, None] * z[None, :], lo, hi) - lo) / delta        # [B, j]
    w = np.maximum(0.0, 1.0 - np.abs(b[:, :, None] - k[None, None, :]))                                # [B, j, k]
    return np.einsum("ij,ijk->ik", pt, w)


def project_scatter(pt, r, g, N, vmin, vmax):
    """The classic floor / ceil scatter of C51 (Bellemare et al. 2017, algorithm 1), which drops the mass of a b_j that is an
    integer: for comparison on inputs where none is."""
    z, lo, hi, delta = support(N, vmin, vmax)
    b = (np.clip(np.asarray(r, np.float64)[:, None] + np.asarray(g, np.float64)[:, None] * z[None, :], lo, hi) - lo) / delta
    l, u = np.floor(b).astype(int), np.ceil(b).astype(int)
    m = np.zeros_like(pt)
    for i in range(pt.shape[0]):
        for j in range(N):
            m[i, l[i, j]] += pt[i, j] * (u[i, j] - b[i, j])
            m[i, u[i, j]] += pt[i, j] * (b[i, j] - l[i, j])
    return m


def targets(T, s2, r, done, gamma, N, vmin, vmax, future=True):
    """Steps 1-2 -> dict(pt, m, y, qt, g).  gamma: a scalar or the rows' discounts [B]."""
    dtype = T["critic_fc1/W"].dtype.type
    z = support(N, vmin, vmax, dtype)[0]
    r = np.asarray(r, dtype)
    B = r.shape[0]
    if not future:
        m = project(None, r, None, N, vmin, vmax).astype(dtype)
        return dict(pt=np.zeros((B, N), dtype), m=m, y=m @ z, qt=np.zeros(B, dtype), g=np.zeros(B, dtype))
    pt = head(T, s2, o.actor_forward(T, s2)["out"])["p"]
    g = np.where(np.asarray(done) != 0, 0.0, np.broadcast_to(np.asarray(gamma, dtype), (B,))).astype(dtype)
    m = project(pt, r, g, N, vmin, vmax)
    return dict(pt=pt, m=m, y=m @ z, qt=pt @ z, g=g)


def critic_grads(P, s, a, m, N, vmin, vmax, w=None):
    """Step 3's gradient of L = (1/B) sum_i w_i ce_i with m held constant -> (forward dict with p, q, ce, dz, dt, dn1; grads of
    the ten trainable variables)."""
    f = head(P, s, a)
    dtype = f["p"].dtype.type
    z = support(N, vmin, vmax, dtype)[0]
    B = f["p"].shape[0]
    wt = np.ones(B, dtype) if w is None else np.asarray(w, dtype)
    ce = -(m * log_softmax(f["q"])).sum(axis=1)
    dz = (wt / dtype(B))[:, None] * (f["p"] - m)
    g = {"critic_output/W": f["c2"].T @ dz, "critic_output/b": dz.sum(0)}
    dt = (dz @ P["critic_output/W"].T) * (f["t"] > 0)
    g["critic_fc2/W"] = f["c1"].T @ dt
    g["critic_norm2/W"] = f["a"].T @ dt
    g["critic_norm2/b"] = dt.sum(0)
    g["critic_fc2/b"] = np.zeros(o.H2, dtype)
    dn1 = (dt @ P["critic_fc2/W"].T) * (f["n1"] > 0)
    g["critic_norm1/beta"] = dn1.sum(0)
    g["critic_norm1/gamma"] = (dn1 * f["xh1"]).sum(0)
    dh1 = dn1 * (P["critic_norm1/gamma"] * f["rs1"])
    g["critic_fc1/W"] = f["x"].T @ dh1
    g["critic_fc1/b"] = dh1.sum(0)
    f.update(logits=f["q"], qv=f["p"] @ z, ce=ce, dz=dz, dt=dt, dn1=dn1, dh1=dh1, loss=(wt * ce).sum() / dtype(B))
    return f, g


def action_gradient(P, s, a, N, vmin, vmax):
    """Step 4: g = dQ/da per row, Q = sum_k z_k p_k."""
    f = head(P, s, a)
    z = support(N, vmin, vmax, f["p"].dtype.type)[0]
    q = f["p"] @ z
    dl = f["p"] * (z[None, :] - q[:, None])
    dt = (dl @ P["critic_output/W"].T) * (f["t"] > 0)
    return dt @ P["critic_norm2/W"].T


def relu_margin(online, target, s, a, s2):
    """ddpg_oracle.relu_margin: the head has no relu, and the projection, the softmax and the clip are continuous."""
    return o.relu_margin(online, target, s, a, s2)


def train_step(st, s, a, r, done, s2, lr, noise=None, *, atoms, vmin, vmax, actor_lr=1.0, critic_lr=10.0, tau=0.001, gamma=0.99,
               future=True, critic_rmsprop=True, decay=0.99, momentum=0.0, eps=0.1, clip=None, stop_after=6, w=None):
    """Steps 1-6 of the distributional step on `st` in place (ddpg_oracle.train_step's state and conventions).  gamma: a scalar
    or the rows' discounts; w: the rows' importance weights (None: 1)."""
    O, T = st["online"], st["target"]
    t = st["step"] + 1
    tg = targets(T, s2, r, done, gamma, atoms, vmin, vmax, future)
    fc, gc = critic_grads(O, s, a, tg["m"], atoms, vmin, vmax, w)
    out = dict(y=tg["y"], qt=tg["qt"], pt=tg["pt"], m=tg["m"], g_row=tg["g"], q=fc["qv"].copy(), p=fc["p"], dz=fc["dz"], ce=fc["ce"],
               loss=fc["loss"], critic_grads=gc, critic_fwd=fc)
    out["q_max"], out["q_avg"] = float(out["q"].max()), float(out["q"].mean())
    for k in CRITIC_TRAINABLE:
        if k == DEAD:
            continue
        g = o.clip_by_norm(gc[k], clip) if clip else gc[k]
        if critic_rmsprop:
            o.rmsprop_step(O[k], st["slot_a"][k], st["slot_b"][k], g, critic_lr * lr, decay, momentum, eps)
        else:
            o.adam_step(O[k], st["slot_a"][k], st["slot_b"][k], g, critic_lr * lr, t)
    if stop_after <= 3:
        return out
    fa0 = o.actor_forward(O, s)
    a_out = fa0["out"] + (0.0 if noise is None else np.asarray(noise, fa0["out"].dtype)[None, :])
    g = action_gradient(O, s, a_out, atoms, vmin, vmax)
    fa, ga = o.actor_grads(O, s, g)
    out.update(a_out=a_out, g=g, actor_grads=ga, actor_fwd=fa)
    if stop_after <= 4:
        return out
    for k in ACTOR_TRAINABLE:
        o.adam_step(O[k], st["slot_a"][k], st["slot_b"][k], ga[k], actor_lr * lr, t)
    o.soft_update(O, T, tau)
    st["step"] = t
    return out
