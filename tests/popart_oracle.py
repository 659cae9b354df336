"""Oracle of PopArt on the DDPG handle's critic (Config.DDPG_POPART; ddpg_popart_kernel and the target kernel's
de-normalisation in csrc/ga3c_ddpg.hip) for the tests (not collected: no test_ prefix).  van Hasselt et al. 2016, "Learning values
across many orders of magnitude", on top of tests/ddpg_oracle.py.

  state    mu, nu: the running first and second moment of the targets, 0 and 1 at first.
           sigma = clamp(sqrt(max(nu - mu^2, 0)), sigma_min, sigma_max).  The critic's output n stands for the return sigma n + mu.
  targets  q' = sigma n' + mu with n' the target critic's output; y = r on a done row or without future reward, else r + g q'.
  update   mu' = (1 - beta) mu + beta mean(y), nu' = (1 - beta) nu + beta mean(y^2), sigma' from them.
  rescale  critic_output/W <- W sigma / sigma', /b <- b sigma / sigma' + (mu - mu') / sigma', online and target: sigma' n + mu' is
           what sigma n + mu was.
  critic   the paired step on yn = (y - mu') / sigma'; actor, soft update and optimizers as ddpg_oracle states them.

Two forms.  float64 throughout is the statement.  The mixed form is the kernel's: mu and nu are stored in f32, the update and
sigma run in f64 on the stored values, and ratio, shift, mu' and 1 / sigma' are rounded to f32 before they meet the f32 weights
and targets, with fmaf where the kernel has it (fmaf32 below is exact).
"""
from fractions import Fraction

import numpy as np

import ddpg_oracle as o
import per_oracle as per

THREADS, LEAVES = 448, 512            # the kernel's workgroup and the leaves of its tree
SIGMA_MIN, SIGMA_MAX = 1e-4, 1e6      # Config's defaults
WO, BO = "critic_output/W", "critic_output/b"


def sigma_of(mu, nu, smin=SIGMA_MIN, smax=SIGMA_MAX):
    """f64, from mu and nu as they are stored."""
    mu, nu = float(mu), float(nu)
    return float(min(max(np.sqrt(max(nu - mu * mu, 0.0)), float(smin)), float(smax)))


def bounds32(smin=SIGMA_MIN, smax=SIGMA_MAX):
    """The clamps as the handle keeps them: f32."""
    return float(np.float32(smin)), float(np.float32(smax))


def fmaf32(a, b, c):
    """fmaf on f32 values, elementwise: a b + c exactly, rounded once to f32 (ties to even)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(c, np.float32))
    out = np.empty(a.shape, np.float32)
    for i in np.ndindex(a.shape):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        r = np.float32(float(exact))              # within one f32 spacing; settle among it and its neighbours
        best = None
        for cand in (np.nextafter(r, np.float32(-np.inf)), r, np.nextafter(r, np.float32(np.inf))):
            if not np.isfinite(cand):
                continue
            d = abs(Fraction(float(cand)) - exact)
            even = (int(np.float32(cand).view(np.uint32)) & 1) == 0
            if best is None or d < best[0] or (d == best[0] and even and not best[2]):
                best = (d, cand, even)
        out[i] = best[1]
    return out if out.shape else np.float32(out)


def kernel_sums(y):
    """-> (sum y, sum y^2) in f64 in the kernel's order: thread t adds rows t, t + 448, .. in that order, the 448 partials and 64
    zeros fold by the halving tree x[t] += x[t + h], h = 256 .. 1."""
    y = np.asarray(y, np.float64).ravel()
    part = np.zeros((2, LEAVES), np.float64)
    for t in range(min(THREADS, y.size)):
        for v in y[t::THREADS]:
            part[0, t] = part[0, t] + v
            part[1, t] = part[1, t] + v * v
    h = LEAVES // 2
    while h > 0:
        part[:, :h] = part[:, :h] + part[:, h:2 * h]
        h //= 2
    return float(part[0, 0]), float(part[1, 0])


def update64(mu, nu, y, beta):
    """The statistics' step in float64, nothing rounded -> (mu', nu')."""
    y = np.asarray(y, np.float64)
    return (1.0 - beta) * mu + beta * float(np.mean(y)), (1.0 - beta) * nu + beta * float(np.mean(y * y))


def update_mixed(mu, nu, y, beta):
    """The kernel's: f32 mu, nu and f32 beta in, the f64 update on the kernel's sums, each result rounded to f32."""
    mu, nu, beta = float(np.float32(mu)), float(np.float32(nu)), float(np.float32(beta))
    y = np.asarray(y, np.float32)
    s1, s2 = kernel_sums(y)
    B = float(y.size)
    return np.float32((1.0 - beta) * mu + beta * (s1 / B)), np.float32((1.0 - beta) * nu + beta * (s2 / B))


def constants(mu, nu, mu1, nu1, smin=SIGMA_MIN, smax=SIGMA_MAX, mixed=True):
    """-> (ratio, shift, muf', isig', sigma, sigma'): what the rescale and yn are made with, from the statistics before and the
    STORED statistics after.  mixed: the clamps and the four constants are f32."""
    if mixed:
        smin, smax = bounds32(smin, smax)
    mu, nu, mu1, nu1 = float(mu), float(nu), float(mu1), float(nu1)
    sigma, sigma1 = sigma_of(mu, nu, smin, smax), sigma_of(mu1, nu1, smin, smax)
    ratio, shift, isig = sigma / sigma1, (mu - mu1) / sigma1, 1.0 / sigma1
    if mixed:
        return np.float32(ratio), np.float32(shift), np.float32(mu1), np.float32(isig), sigma, sigma1
    return ratio, shift, mu1, isig, sigma, sigma1


def rescale(W, b, ratio, shift):
    """critic_output's W and b after the rescale, in the dtype of W: f32 is the kernel's W ratio and fmaf(b, ratio, shift)."""
    if np.asarray(W).dtype == np.float32:
        return np.asarray(W, np.float32) * np.float32(ratio), np.asarray(fmaf32(b, ratio, shift), np.float32).reshape(np.shape(b))
    return W * ratio, b * ratio + shift


def normalise(y, muf, isig):
    """yn = (y - mu') isig' in y's dtype (f32: the kernel's two roundings)."""
    if np.asarray(y).dtype == np.float32:
        return (np.asarray(y, np.float32) - np.float32(muf)) * np.float32(isig)
    return (y - muf) * isig


def new_state(online, target, critic_rmsprop=True, mu=0.0, nu=1.0):
    st = o.new_state(online, target, critic_rmsprop)
    st.update(mu=mu, nu=nu)
    return st


def preserved(P, c2, mu, nu, y, beta, smin=SIGMA_MIN, smax=SIGMA_MAX, mixed=True):
    """One statistics jump on a head (W, b) = P and its inputs c2 [B,300] -> (return-scale outputs before, after, state after).
    mixed: everything the kernel holds in f32 is f32 here (the head's sum too, in numpy's order); the two returns are formed in
    f64 from those values, as a test forms them from what it fetches."""
    W, b = P
    if mixed:
        W, b, c2 = np.asarray(W, np.float32), np.asarray(b, np.float32), np.asarray(c2, np.float32)
        mu, nu = np.float32(mu), np.float32(nu)
        mu1, nu1 = update_mixed(mu, nu, y, beta)
    else:
        mu1, nu1 = update64(mu, nu, y, beta)
    ratio, shift, _, _, sigma, sigma1 = constants(mu, nu, mu1, nu1, smin, smax, mixed)
    n0 = (c2 @ W + b)[:, 0]
    W1, b1 = rescale(W, b, ratio, shift)
    n1 = (c2 @ W1 + b1)[:, 0]
    before = sigma * n0.astype(np.float64) + float(mu)
    after = sigma1 * n1.astype(np.float64) + float(mu1)
    return before, after, (W1, b1, mu1, nu1)


def train_step(st, s, a, r, done, s2, lr, noise=None, *, beta, smin=SIGMA_MIN, smax=SIGMA_MAX, mixed=False, w=None, disc=None,
               actor_lr=1.0, critic_lr=10.0, tau=0.001, gamma=0.99, future=True, critic_rmsprop=True, decay=0.99, momentum=0.0,
               eps=0.1, clip=None, stop_after=6):
    """ddpg_oracle.train_step's paired step with PopArt, on `st` in place (new_state above).  w: None or the importance weights
    [B] of a prioritised step; disc: None or the rows' discounts [B] of a step on n-step rows.  mixed: the networks stay in the
    dtype of their weights, the statistics are stored in f32 and the constants are f32.
    -> dict(y, qt, yn, q (normalised), dq, q_max, q_avg (return units), mu, nu, sigma, critic_grads, ...)."""
    O, T = st["online"], st["target"]
    t = st["step"] + 1
    mu, nu = st["mu"], st["nu"]
    lo, hi = bounds32(smin, smax) if mixed else (smin, smax)
    sigma = sigma_of(mu, nu, lo, hi)
    r = np.asarray(r, T["critic_fc1/W"].dtype)
    if future:
        nt = o.critic_forward(T, s2, o.actor_forward(T, s2)["out"])["q"][:, 0]
        qt = (np.float32(sigma) if mixed else sigma) * nt + (np.float32(mu) if mixed else mu)
        g = gamma if disc is None else np.asarray(disc, qt.dtype)
        y = np.where(np.asarray(done) != 0, r, r + g * qt)
    else:
        y, qt = r.copy(), None
    if mixed:
        mu1, nu1 = update_mixed(mu, nu, y, beta)
    else:
        mu1, nu1 = update64(mu, nu, y, beta)
    ratio, shift, muf, isig, _, sigma1 = constants(mu, nu, mu1, nu1, smin, smax, mixed)
    for P in (O, T):
        P[WO], P[BO] = rescale(P[WO], P[BO], ratio, shift)
    yn = normalise(y, muf, isig)
    st["mu"], st["nu"] = mu1, nu1
    if w is None:
        fc, dq, gc = o.critic_grads(O, s, a, yn, "paired")
    else:
        fc, dq, gc = per.critic_grads(O, s, a, yn, w)
    out = dict(y=y, qt=qt, yn=yn, q=fc["q"][:, 0].copy(), dq=dq, critic_grads=gc, critic_fwd=fc, mu=mu1, nu=nu1, sigma=sigma1)
    out["q_max"] = float(sigma1 * out["q"].max() + float(mu1))
    out["q_avg"] = float(sigma1 * out["q"].mean() + float(mu1))
    for k in o.CRITIC_TRAINABLE:
        if k == o.DEAD:
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
    g = o.action_gradient(O, s, a_out)
    fa, ga = o.actor_grads(O, s, g)
    out.update(a_out=a_out, g=g, actor_grads=ga, actor_fwd=fa)
    if stop_after <= 4:
        return out
    for k in o.ACTOR_TRAINABLE:
        o.adam_step(O[k], st["slot_a"][k], st["slot_b"][k], ga[k], actor_lr * lr, t)
    o.soft_update(O, T, tau)
    st["step"] = t
    return out
