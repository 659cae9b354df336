"""f64 statement of the DDPG handle's twin step (Config.DDPG_TWIN, ga3c_ddpg_twin_create) for the tests (not
collected: no test_ prefix): clipped double-Q with target policy smoothing and a delayed policy update (Fujimoto et al.
2018), on top of tests/ddpg_oracle.py.  Critic 2 is the critic's network under the names critic2_*; critic2() shows its
variables under the critic's names, so ddpg_oracle's critic_forward / critic_grads / action_gradient serve both.

With t = step + 1:
  1. a~ = clip(actor_target(s2) + eps, -1, 1), eps[k][i] = (f32) clip(sigma n[k][i], -c, c), n Box-Muller in f64 on the
     device's counter uniforms (device_agents_oracle.uniform): j = k A + i, u1 = 1 - u(seed, t, 2j), u2 = u(seed, t, 2j + 1),
     n = sqrt(-2 ln u1) cos(2 pi u2).
  2. q' = min(critic_target(s2, a~), critic2_target(s2, a~)); y from it as ddpg_oracle.targets.
  3. Both critics step on y in the paired form, dq_i = (2/B) w_i (q_i - y_i), each with its own slots and clip_by_norm.
  4. Only when t % policy_delay == 0: ddpg_oracle's steps 4-5 against the updated critic 1, the actor's Adam at count
     t / policy_delay, and the soft update of all three nets.
As in ddpg_oracle every function follows the dtype of the weights it is given.
"""
import numpy as np

import ddpg_oracle as o
import device_agents_oracle as da

_C = len("critic_")
CRITIC2_TRAINABLE = tuple("critic2_" + k[_C:] for k in o.CRITIC_TRAINABLE)
CRITIC2_STATS = ("critic2_norm1/moving_mean", "critic2_norm1/moving_variance")
TRAINABLE = o.TRAINABLE + CRITIC2_TRAINABLE
ALL_VARS = o.ALL_VARS + CRITIC2_TRAINABLE + CRITIC2_STATS         # the engine's order: the 26, then the twin's 12
DEAD2 = "critic2_" + o.DEAD[_C:]


def critic2(P):
    """Critic 2's variables of P under the critic's names: the same arrays, so a step in place is a step on P."""
    return {"critic_" + k[len("critic2_"):]: v for k, v in P.items() if k.startswith("critic2_")}


def shapes(S, A):
    sh = o.shapes(S, A)
    sh.update({k2: sh[k] for k, k2 in zip(o.CRITIC_TRAINABLE, CRITIC2_TRAINABLE)})
    sh.update({k: (o.H1,) for k in CRITIC2_STATS})
    return sh


def random_params(S, A, rng, scale=0.3, stats=False):
    """ddpg_oracle.random_params' 26, then critic 2's 12 from the same rules, drawn after them."""
    p = o.random_params(S, A, rng, scale, stats)
    second = o.random_params(S, A, rng, scale, stats)
    for k in o.CRITIC_TRAINABLE + ("critic_norm1/moving_mean", "critic_norm1/moving_variance"):
        p["critic2_" + k[_C:]] = second[k]
    return p


def smoothing_noise(seed, t, B, A, sigma, c):
    """eps [B, A] float32 of step t (statement 1 above)."""
    j = np.arange(B * A, dtype=np.uint64)
    u1 = 1.0 - da.uniform(seed, t, 2 * j)
    u2 = da.uniform(seed, t, 2 * j + 1)
    n = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    sigma, c = float(np.float32(sigma)), float(np.float32(c))
    return np.clip(sigma * n, -c, c).astype(np.float32).reshape(B, A)


def target_action(T, s2, eps):
    out = o.actor_forward(T, s2)["out"]
    return np.clip(out + np.asarray(eps, out.dtype), -1.0, 1.0)


def targets(T, s2, r, done, gamma, eps, future=True):
    """Steps 1-2 -> (y, qt = min, qt1, qt2, a~)."""
    r = np.asarray(r, T["critic_fc1/W"].dtype)
    if not future:
        return r.copy(), None, None, None, None
    at = target_action(T, s2, eps)
    qt1 = o.critic_forward(T, s2, at)["q"][:, 0]
    qt2 = o.critic_forward(critic2(T), s2, at)["q"][:, 0]
    qt = np.minimum(qt1, qt2)
    return np.where(np.asarray(done) != 0, r, r + gamma * qt), qt, qt1, qt2, at


def relu_margin(online, target, s, a, s2, eps):
    """Per row: the smallest |pre-activation| of any relu unit in the six evaluations of a twin step: ddpg_oracle.relu_margin's
    actor(s), critic(s, a), actor_target(s2), and critic2(s, a) and both target critics at the smoothed action."""
    fa = o.actor_forward(online, s)
    ft = o.actor_forward(target, s2)
    at = target_action(target, s2, eps)
    fs = [(fa, ("n1", "n2")), (ft, ("n1", "n2")), (o.critic_forward(online, s, a), ("n1", "t")),
          (o.critic_forward(critic2(online), s, a), ("n1", "t")), (o.critic_forward(target, s2, at), ("n1", "t")),
          (o.critic_forward(critic2(target), s2, at), ("n1", "t"))]
    return np.min([np.abs(f[k]).min(axis=1) for f, ks in fs for k in ks], axis=0)


def new_state(online, target, critic_rmsprop=True):
    """ddpg_oracle.new_state over the 30 trainable variables."""
    st = dict(online={k: v.copy() for k, v in online.items()}, target={k: v.copy() for k, v in target.items()},
              slot_a={}, slot_b={}, step=0)
    for k in TRAINABLE:
        rms = critic_rmsprop and k not in o.ACTOR_TRAINABLE
        st["slot_a"][k] = np.ones_like(online[k]) if rms else np.zeros_like(online[k])
        st["slot_b"][k] = np.zeros_like(online[k])
    return st


def train_step(st, s, a, r, done, s2, lr, noise=None, *, policy_delay=2, sigma=0.2, noise_clip=0.5, seed=0, eps=None, per_w=None,
               actor_lr=1.0, critic_lr=10.0, tau=0.001, gamma=0.99, future=True, critic_rmsprop=True, decay=0.99, momentum=0.0,
               rms_eps=0.1, clip=None, stop_after=6):
    """One twin step on `st` in place.  eps: the smoothing noise [B, A] if given (the device's, fetched), else drawn.  per_w:
    importance weights [B] or None.  -> dict; stop_after as ddpg_oracle.train_step's, 4 doing what 3 does off a policy step."""
    O, T = st["online"], st["target"]
    t = st["step"] + 1
    policy = t % policy_delay == 0
    B, A = np.shape(a)
    if eps is None:
        eps = smoothing_noise(seed, t, B, A, sigma, noise_clip)
    y, qt, qt1, qt2, at = targets(T, s2, r, done, gamma, eps, future)
    out = dict(y=y, qt=qt, qt1=qt1, qt2=qt2, t_a=at, t_eps=np.asarray(eps), policy=policy)
    for tag, P, pre in (("", O, "critic_"), ("2", critic2(O), "critic2_")):
        f, dq, g = o.critic_grads(P, s, a, y, "paired") if per_w is None else _weighted(P, s, a, y, per_w)
        out["q" + tag], out["dq" + tag], out["critic%s_grads" % tag], out["critic%s_fwd" % tag] = f["q"][:, 0].copy(), dq, g, f
        for k in o.CRITIC_TRAINABLE:
            if k == o.DEAD:
                continue
            gk = o.clip_by_norm(g[k], clip) if clip else g[k]
            name = pre + k[_C:]
            if critic_rmsprop:
                o.rmsprop_step(P[k], st["slot_a"][name], st["slot_b"][name], gk, critic_lr * lr, decay, momentum, rms_eps)
            else:
                o.adam_step(P[k], st["slot_a"][name], st["slot_b"][name], gk, critic_lr * lr, t)
    out["q_max"], out["q_avg"] = float(out["q"].max()), float(out["q"].mean())
    if stop_after <= 3 or (not policy and stop_after <= 4):
        return out
    if policy:
        fa0 = o.actor_forward(O, s)
        a_out = fa0["out"] + (0.0 if noise is None else np.asarray(noise, fa0["out"].dtype)[None, :])
        g = o.action_gradient(O, s, a_out)
        fa, ga = o.actor_grads(O, s, g)
        out.update(a_out=a_out, g=g, actor_grads=ga, actor_fwd=fa)
        if stop_after <= 4:
            return out
        for k in o.ACTOR_TRAINABLE:
            o.adam_step(O[k], st["slot_a"][k], st["slot_b"][k], ga[k], actor_lr * lr, t // policy_delay)
        for k in TRAINABLE:
            T[k] = tau * O[k] + (1.0 - tau) * T[k]
    st["step"] = t
    return out


def _weighted(P, s, a, y, w):
    """critic_grads with dq_i = (2/B) w_i (q_i - y_i), as per_oracle.critic_grads states it: the paired form on
    y' = q - w (q - y)."""
    q = o.critic_forward(P, s, a)["q"][:, 0]
    return o.critic_grads(P, s, a, q - np.asarray(w, q.dtype) * (q - np.asarray(y, q.dtype)), "paired")
