"""f64 statement of the DDPG networks and their train step for the tests (not collected: no test_ prefix).

Reference NetworkDDPG.py (USE_DDPG with CONTINUOUS_INPUT), restated in DESIGN.md 8f:
    actor   x -> actor_fc1 (400) -> actor_norm1 -> relu -> actor_fc2 (300) -> actor_norm2 -> relu -> actor_output (A, tanh)
    critic  x -> critic_fc1 (400) -> critic_norm1 -> relu = h;  q = critic_output(relu(h W_fc2 + a W_n2 + b_n2)), where
            W_n2, b_n2 are the dense layer the reference names critic_norm2; critic_fc2/b is a variable no graph reads.
    train_DDPG (:64-98): targets from the target nets, critic step, action gradient of the updated critic, actor step,
    soft update of both target nets.

Batch normalisation is the inference form only (the reference never switches tflearn's training flag on), stated once
in bn(): gamma (x - moving_mean) / sqrt(moving_variance + BN_EPS) + beta.

Every function follows the dtype of the weights it is given: float64 is the statement, float32 weights give the
like-for-like restatement that tests/closeness.py's bound is measured with.
"""
import numpy as np

H1, H2 = 400, 300
BN_EPS = 1e-5
ADAM_B1, ADAM_B2, ADAM_EPS = 0.9, 0.999, 1e-8

ACTOR_TRAINABLE = ("actor_fc1/W", "actor_fc1/b", "actor_norm1/beta", "actor_norm1/gamma", "actor_fc2/W", "actor_fc2/b",
                   "actor_norm2/beta", "actor_norm2/gamma", "actor_output/W", "actor_output/b")
CRITIC_TRAINABLE = ("critic_fc1/W", "critic_fc1/b", "critic_norm1/beta", "critic_norm1/gamma", "critic_fc2/W", "critic_fc2/b",
                    "critic_norm2/W", "critic_norm2/b", "critic_output/W", "critic_output/b")
STATS = ("actor_norm1/moving_mean", "actor_norm1/moving_variance", "actor_norm2/moving_mean", "actor_norm2/moving_variance",
         "critic_norm1/moving_mean", "critic_norm1/moving_variance")
TRAINABLE = ACTOR_TRAINABLE + CRITIC_TRAINABLE
ALL_VARS = TRAINABLE + STATS          # the engine's arena order
DEAD = "critic_fc2/b"                 # in no forward pass (NetworkDDPG.py:390-392): no gradient, the optimizer skips it


def shapes(S, A):
    return {"actor_fc1/W": (S, H1), "actor_fc1/b": (H1,), "actor_norm1/beta": (H1,), "actor_norm1/gamma": (H1,),
            "actor_fc2/W": (H1, H2), "actor_fc2/b": (H2,), "actor_norm2/beta": (H2,), "actor_norm2/gamma": (H2,),
            "actor_output/W": (H2, A), "actor_output/b": (A,),
            "critic_fc1/W": (S, H1), "critic_fc1/b": (H1,), "critic_norm1/beta": (H1,), "critic_norm1/gamma": (H1,),
            "critic_fc2/W": (H1, H2), "critic_fc2/b": (H2,), "critic_norm2/W": (A, H2), "critic_norm2/b": (H2,),
            "critic_output/W": (H2, 1), "critic_output/b": (1,),
            "actor_norm1/moving_mean": (H1,), "actor_norm1/moving_variance": (H1,),
            "actor_norm2/moving_mean": (H2,), "actor_norm2/moving_variance": (H2,),
            "critic_norm1/moving_mean": (H1,), "critic_norm1/moving_variance": (H1,)}


def random_params(S, A, rng, scale=0.3, stats=False):
    """Test weights, U(-scale, scale), f32-rounded; gamma around 1; moving statistics 0 / 1 unless `stats`."""
    p = {}
    for k, sh in shapes(S, A).items():
        if k.endswith("moving_mean"):
            v = rng.uniform(-0.5, 0.5, sh) if stats else np.zeros(sh)
        elif k.endswith("moving_variance"):
            v = rng.uniform(0.5, 2.0, sh) if stats else np.ones(sh)
        elif k.endswith("gamma"):
            v = rng.uniform(0.7, 1.3, sh)
        else:
            v = rng.uniform(-scale, scale, sh)
        p[k] = v.astype(np.float32).astype(np.float64)
    return p


def bn(P, name, h):
    """-> (xhat, rstd, n): the one statement of the reference's batch normalisation (inference form)."""
    rstd = 1.0 / np.sqrt(P[name + "/moving_variance"] + BN_EPS)
    xhat = (h - P[name + "/moving_mean"]) * rstd
    return xhat, rstd, P[name + "/gamma"] * xhat + P[name + "/beta"]


def actor_forward(P, x):
    x = np.asarray(x, P["actor_fc1/W"].dtype)
    h1 = x @ P["actor_fc1/W"] + P["actor_fc1/b"]
    xh1, rs1, n1 = bn(P, "actor_norm1", h1)
    a1 = np.maximum(n1, 0.0)
    h2 = a1 @ P["actor_fc2/W"] + P["actor_fc2/b"]
    xh2, rs2, n2 = bn(P, "actor_norm2", h2)
    a2 = np.maximum(n2, 0.0)
    ho = a2 @ P["actor_output/W"] + P["actor_output/b"]
    return dict(x=x, h1=h1, xh1=xh1, rs1=rs1, n1=n1, a1=a1, h2=h2, xh2=xh2, rs2=rs2, n2=n2, a2=a2, ho=ho, out=np.tanh(ho))


def dtanh(h):
    """1 - tanh(h)^2 = 1 / cosh(h)^2 as 4 e / (1 + e)^2 with e = exp(-2 |h|), in h's dtype: from the pre-activation, no
    subtraction, so it keeps its RELATIVE accuracy however far the unit is saturated (and e, at most 1, cannot overflow)."""
    e = np.exp(-2.0 * np.abs(h))
    return 4.0 * e / ((1.0 + e) * (1.0 + e))


def critic_forward(P, x, a):
    x, a = np.asarray(x, P["critic_fc1/W"].dtype), np.asarray(a, P["critic_fc1/W"].dtype)
    h1 = x @ P["critic_fc1/W"] + P["critic_fc1/b"]
    xh1, rs1, n1 = bn(P, "critic_norm1", h1)
    c1 = np.maximum(n1, 0.0)
    t = c1 @ P["critic_fc2/W"] + a @ P["critic_norm2/W"] + P["critic_norm2/b"]
    c2 = np.maximum(t, 0.0)
    q = c2 @ P["critic_output/W"] + P["critic_output/b"]              # [B, 1]
    return dict(x=x, a=a, h1=h1, xh1=xh1, rs1=rs1, n1=n1, c1=c1, t=t, c2=c2, q=q)


def relu_margin(online, target, s, a, s2):
    """Per row: the smallest |pre-activation| of any relu unit in the four nets as a step evaluates them first: actor(s),
    critic(s, a), actor_target(s2), critic_target(s2, .).  The GPU tests leave out rows where f32 could land on the other
    side of zero."""
    fa = actor_forward(online, s)
    at = actor_forward(target, s2)
    ct = critic_forward(target, s2, at["out"])
    c = critic_forward(online, s, a)
    m = [np.abs(f[k]).min(axis=1) for f, ks in ((fa, ("n1", "n2")), (at, ("n1", "n2")), (ct, ("n1", "t")), (c, ("n1", "t")))
         for k in ks]
    return np.min(m, axis=0)


def targets(T, s2, r, done, gamma, future=True):
    """Steps 1-2: y_i = r_i if done_i else r_i + gamma q'_i;  q' = critic_target(s2, actor_target(s2))."""
    r = np.asarray(r, T["critic_fc1/W"].dtype)
    if not future:
        return r.copy(), None
    qt = critic_forward(T, s2, actor_forward(T, s2)["out"])["q"][:, 0]
    return np.where(np.asarray(done) != 0, r, r + gamma * qt), qt


def critic_grads(P, s, a, y, form="fork"):
    """Step 3's gradient.  'fork': tflearn.mean_square(y[B], q[B,1]) broadcasts to [B,B]: dL/dq_i = (2/B)(q_i - mean(y)).
    'paired': dL/dq_i = (2/B)(q_i - y_i).  -> (forward dict, dq [B], grads of the ten trainable variables)."""
    f = critic_forward(P, s, a)
    B = f["q"].shape[0]
    q = f["q"][:, 0]
    ref = np.mean(y) if form == "fork" else np.asarray(y, q.dtype)
    dq = (2.0 / B) * (q - ref)
    g = {}
    g["critic_output/W"] = f["c2"].T @ dq[:, None]
    g["critic_output/b"] = np.array([dq.sum()])
    dt = (dq[:, None] * P["critic_output/W"][:, 0][None, :]) * (f["t"] > 0)
    g["critic_fc2/W"] = f["c1"].T @ dt
    g["critic_norm2/W"] = f["a"].T @ dt
    g["critic_norm2/b"] = dt.sum(0)
    g["critic_fc2/b"] = np.zeros(H2, q.dtype)
    dn1 = (dt @ P["critic_fc2/W"].T) * (f["n1"] > 0)
    g["critic_norm1/beta"] = dn1.sum(0)
    g["critic_norm1/gamma"] = (dn1 * f["xh1"]).sum(0)
    dh1 = dn1 * (P["critic_norm1/gamma"] * f["rs1"])
    g["critic_fc1/W"] = f["x"].T @ dh1
    g["critic_fc1/b"] = dh1.sum(0)
    f.update(dq=dq, dt=dt, dn1=dn1)
    return f, dq, g


def action_gradient(P, s, a):
    """Step 4: g = dq/da per row, no 1/B (tf.gradients(out, action), :89)."""
    f = critic_forward(P, s, a)
    dt = P["critic_output/W"][:, 0][None, :] * (f["t"] > 0)
    return dt @ P["critic_norm2/W"].T


def actor_grads(P, s, g):
    """Step 5: d(out)/d(var) contracted with -g, summed over rows (:182-183).  The output's derivative is taken from its
    pre-activation (dtanh), not as 1 - out^2: tanh rounds to within an ulp of 1 from |h| = 9 (float32) or 19 (float64) on, and
    1 - out^2 is then zero or a multiple of the ulp where the derivative, 4 exp(-2 |h|), is neither -- wrong by 100 % of a
    saturated unit's delta, which the engine computes from h and which a test can only hold it to if this statement does."""
    f = actor_forward(P, s)
    do = -np.asarray(g, f["out"].dtype) * dtanh(f["ho"])
    G = {"actor_output/W": f["a2"].T @ do, "actor_output/b": do.sum(0)}
    dn2 = (do @ P["actor_output/W"].T) * (f["n2"] > 0)
    G["actor_norm2/beta"] = dn2.sum(0)
    G["actor_norm2/gamma"] = (dn2 * f["xh2"]).sum(0)
    dh2 = dn2 * (P["actor_norm2/gamma"] * f["rs2"])
    G["actor_fc2/W"] = f["a1"].T @ dh2
    G["actor_fc2/b"] = dh2.sum(0)
    dn1 = (dh2 @ P["actor_fc2/W"].T) * (f["n1"] > 0)
    G["actor_norm1/beta"] = dn1.sum(0)
    G["actor_norm1/gamma"] = (dn1 * f["xh1"]).sum(0)
    dh1 = dn1 * (P["actor_norm1/gamma"] * f["rs1"])
    G["actor_fc1/W"] = f["x"].T @ dh1
    G["actor_fc1/b"] = dh1.sum(0)
    f.update(do=do, dn2=dn2, dn1=dn1)
    return f, G


def clip_by_norm(g, clip):
    """tf.clip_by_norm: g * clip / max(||g||_2, clip)."""
    return g * (clip / max(float(np.sqrt(np.sum(g * g))), clip))


def rmsprop_step(theta, ms, mom, g, lr, decay, momentum, eps):
    """TF-1 ApplyRMSProp, in place: ms += (g g - ms)(1 - decay); mom = mom momentum + g lr / sqrt(eps + ms); theta -= mom."""
    ms += (g * g - ms) * (1.0 - decay)
    mom *= momentum
    mom += g * lr / np.sqrt(eps + ms)
    theta -= mom


def adam_step(theta, m, v, g, lr, t):
    """TF-1 ApplyAdam at step t >= 1, in place."""
    lr_t = lr * np.sqrt(1.0 - ADAM_B2 ** t) / (1.0 - ADAM_B1 ** t)
    m += (g - m) * (1.0 - ADAM_B1)
    v += (g * g - v) * (1.0 - ADAM_B2)
    theta -= lr_t * m / (np.sqrt(v) + ADAM_EPS)


def soft_update(online, target, tau):
    """Step 6, every trainable variable (the dead one too): target = tau online + (1 - tau) target."""
    for k in TRAINABLE:
        target[k] = tau * online[k] + (1.0 - tau) * target[k]


def new_state(online, target, critic_rmsprop=True):
    """slot_a / slot_b: RMSProp ms (1) / mom (0) for the critic under RMSPROP, Adam m / v (0) otherwise and for the actor."""
    st = dict(online={k: v.copy() for k, v in online.items()}, target={k: v.copy() for k, v in target.items()},
              slot_a={}, slot_b={}, step=0)
    for k in TRAINABLE:
        rms = critic_rmsprop and k in CRITIC_TRAINABLE
        st["slot_a"][k] = np.ones_like(online[k]) if rms else np.zeros_like(online[k])
        st["slot_b"][k] = np.zeros_like(online[k])
    return st


def train_step(st, s, a, r, done, s2, lr, noise=None, *, actor_lr=1.0, critic_lr=10.0, tau=0.001, gamma=0.99, future=True,
               form="fork", critic_rmsprop=True, decay=0.99, momentum=0.0, eps=0.1, clip=None, stop_after=6):
    """Steps 1-6 of train_DDPG on `st` in place.  noise: None or [A], added to every row of actor(s) in step 4.
    -> dict(y, q, q_max, q_avg, a_out, g, critic_grads, actor_grads); stop_after = 3 / 4 leaves the later steps undone."""
    O, T = st["online"], st["target"]
    t = st["step"] + 1
    y, qt = targets(T, s2, r, done, gamma, future)
    fc, dq, gc = critic_grads(O, s, a, y, form)
    out = dict(y=y, qt=qt, q=fc["q"][:, 0].copy(), dq=dq, critic_grads=gc, critic_fwd=fc)
    out["q_max"], out["q_avg"] = float(out["q"].max()), float(out["q"].mean())
    for k in CRITIC_TRAINABLE:
        if k == DEAD:
            continue
        g = clip_by_norm(gc[k], clip) if clip else gc[k]
        if critic_rmsprop:
            rmsprop_step(O[k], st["slot_a"][k], st["slot_b"][k], g, critic_lr * lr, decay, momentum, eps)
        else:
            adam_step(O[k], st["slot_a"][k], st["slot_b"][k], g, critic_lr * lr, t)
    if stop_after <= 3:
        return out
    fa0 = actor_forward(O, s)
    a_out = fa0["out"] + (0.0 if noise is None else np.asarray(noise, fa0["out"].dtype)[None, :])
    g = action_gradient(O, s, a_out)
    fa, ga = actor_grads(O, s, g)
    out.update(a_out=a_out, g=g, actor_grads=ga, actor_fwd=fa)
    if stop_after <= 4:
        return out
    for k in ACTOR_TRAINABLE:
        adam_step(O[k], st["slot_a"][k], st["slot_b"][k], ga[k], actor_lr * lr, t)
    soft_update(O, T, tau)
    st["step"] = t
    return out


def wrap(v, lo=-1.0, hi=1.0):
    """check_bounds(value, 1, -1, turnaround=True) (NetworkDDPG.py:254-267), elementwise."""
    v = np.array(v, np.float64)
    size = hi - lo
    below, above = v < lo, v > hi
    out = v.copy()
    out[below] = hi - ((lo - v[below]) % size)
    out[above] = ((v[above] - hi) % size) + lo
    return out


def ou_step(x, n, sigma=0.3, theta=0.15, dt=1e-2, mu=0.0):
    """OrnsteinUhlenbeckActionNoise.__call__ (:470-476) given the normal draws n."""
    return x + theta * (mu - x) * dt + sigma * np.sqrt(dt) * n


class Ring:
    """The replay ring's bookkeeping as the engine keeps it: position j of the reference's deque is slot (oldest + j) mod cap."""

    def __init__(self, capacity):
        self.capacity, self.total = int(capacity), 0

    @property
    def size(self):
        return min(self.total, self.capacity)

    @property
    def oldest(self):
        return self.total % self.capacity if self.total > self.capacity else 0

    def add(self, n=1):
        first = self.total % self.capacity
        self.total += n
        return [(first + i) % self.capacity for i in range(n)]

    def slot(self, position):
        return (self.oldest + position) % self.capacity
