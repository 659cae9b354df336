"""Oracle of proportional prioritised replay on the DDPG handle (Config.PRIORITIZED_REPLAY; the per_* kernels of
csrc/ga3c_ddpg.hip) for the tests (not collected: no test_ prefix).  Schaul et al. 2016, the proportional variant, with the
sum recomputed at every draw instead of a sum tree.

Every addition that decides a slot is stated in the order the device makes it, in f64, so the device's slots can be held
to this file exactly:

  state   pa[capacity] f32, a slot's priority already raised to alpha (0 in a slot never written); max_pa f32, 1 at first,
          never smaller; a sample counter.
  fill    the slots a replay_add writes get max_pa.
  sum     size = min(total, capacity) rows in slots 0 .. size-1; a chunk is 1024 consecutive slots.  Of a chunk's 256
          partials, partial t = ((pa[t] + pa[t+256]) + pa[t+512]) + pa[t+768] (slots >= size count 0); they fold by the halving
          tree x[t] += x[t+h], h = 128 .. 1.  The chunk sums, padded with zeros to 1024, get an inclusive Hillis-Steele scan:
          d = 1, 2, 4 .. 512, x[i] += x_old[i-d] for i >= d.  total_pa is the scan's element of the last chunk.
  draw    stratified: u_k = uniform(seed, sample number, k) (tests/device_agents_oracle.py, the sample number in the
          environment's place); target_k = (k + u_k) * (total_pa / B).  The chunk is the first whose scanned sum exceeds
          target_k, the last chunk if none does.  From acc = the scanned sum of the chunk before (0 for chunk 0), acc += pa[j]
          over the chunk's slots in order; the slot is the first j with target_k < acc, and the chunk's last slot below size
          if the walk ends without one (the tree and the walk associate differently).  A slot may come up more than once.
  weight  w_k = (size * pa[slot_k] / total_pa) ** -beta_is in f64, over the largest w of the batch, cast to f32.
  loss    dL/dq_i = (2/B) w_i (q_i - y_i): the gradient of mean(w (y - q)^2), the 'paired' form times the weight.
  update  td_i = |y_i - q_i| (f32); pa[slot_i] = (td_i + eps) ** alpha, the LAST row in batch order where a slot occurs more
          than once; max_pa = max(max_pa, every new priority, those of overwritten rows too).
"""
import numpy as np

import ddpg_oracle as o
import device_agents_oracle as dao

CHUNK = 1024
MAX_CHUNKS = 1024
MAX_CAPACITY = CHUNK * MAX_CHUNKS


def chunk_sums(pa, size):
    """-> f64 [ceil(size / 1024)]: the chunk sums in the device's order of additions."""
    n = (size + CHUNK - 1) // CHUNK
    x = np.zeros(n * CHUNK, np.float64)
    x[:size] = np.asarray(pa[:size], np.float64)
    x = x.reshape(n, 4, 256)
    part = (((0.0 + x[:, 0]) + x[:, 1]) + x[:, 2]) + x[:, 3]
    h = 128
    while h > 0:
        part[:, :h] = part[:, :h] + part[:, h:2 * h]
        h //= 2
    return part[:, 0].copy()


def scan(sums):
    """Inclusive Hillis-Steele scan of the chunk sums padded to 1024 -> the first len(sums) elements."""
    x = np.zeros(MAX_CHUNKS, np.float64)
    x[:len(sums)] = sums
    d = 1
    while d < MAX_CHUNKS:
        y = x.copy()
        y[d:] = x[d:] + x[:-d]
        x = y
        d *= 2
    return x[:len(sums)]


def walk(pa, size, sc, target):
    """-> (slot, clamped): the chunk search and the walk within the chunk for one target."""
    over = np.flatnonzero(target < sc)
    c = int(over[0]) if over.size else len(sc) - 1
    acc = float(sc[c - 1]) if c else 0.0
    lo, hi = c * CHUNK, min(size, (c + 1) * CHUNK)
    for j in range(lo, hi):
        acc = acc + float(pa[j])
        if target < acc:
            return j, False
    return hi - 1, True


def draw(pa, size, batch, seed, number):
    """Sample `number` -> (slots int32 [batch], total_pa, rows that took the clamp)."""
    assert 1 <= size <= len(pa) and batch >= 1
    sc = scan(chunk_sums(pa, size))
    total = float(sc[-1])
    seg = total / float(batch)
    slots, clamped = np.empty(batch, np.int32), 0
    u = dao.uniform(seed, number, np.arange(batch))
    for k in range(batch):
        target = (float(k) + float(u[k])) * seg
        slots[k], cl = walk(pa, size, sc, target)
        clamped += cl
    return slots, total, clamped


def weights(pa, size, slots, total, beta_is):
    w = (float(size) * np.asarray(pa, np.float64)[slots] / total) ** -float(beta_is)
    return (w / w.max()).astype(np.float32)


def sample(pa, size, batch, seed, number, beta_is):
    """-> (slots, weights f32): what ga3c_ddpg_sample_prioritized returns for sample `number`."""
    slots, total, _ = draw(pa, size, batch, seed, number)
    return slots, weights(pa, size, slots, total, beta_is)


def fill(pa, max_pa, total, n):
    """The n rows appended to a ring that has had `total` rows get max_pa, in place."""
    cap = len(pa)
    for i in range(n):
        pa[(total + i) % cap] = np.float32(max_pa)


def new_priorities(y, q, eps, alpha):
    """-> (td f32 [B], pa f64 [B]): |y - q| as the device keeps it, and (td + eps) ** alpha."""
    td = np.abs(np.asarray(y, np.float32) - np.asarray(q, np.float32))
    return td, (td.astype(np.float64) + float(np.float32(eps))) ** float(np.float32(alpha))


def update(pa, max_pa, slots, y, q, eps, alpha):
    """The priority update in place -> the new max_pa.  Rows are stored in batch order, so the last one wins a slot."""
    td, p = new_priorities(y, q, eps, alpha)
    for s, v in zip(slots, p):
        pa[int(s)] = np.float32(v)
    return max(np.float32(max_pa), np.float32(p.max()))


def weighted_dq(q, y, w):
    """dL/dq of mean(w (y - q)^2) with y, q, w of one shape [B]."""
    q = np.asarray(q, np.float64)
    return (2.0 / q.shape[0]) * np.asarray(w, np.float64) * (q - np.asarray(y, np.float64))


def critic_grads(P, s, a, y, w):
    """ddpg_oracle.critic_grads under the weighted loss.  Its 'paired' form is (2/B)(q - y'): with y' = q - w (q - y) that
    is (2/B) w (q - y), to the last bits of q (1e-16 of it, far below any tolerance here)."""
    q = o.critic_forward(P, s, a)["q"][:, 0]
    y = np.asarray(y, q.dtype)
    f, dq, g = o.critic_grads(P, s, a, q - np.asarray(w, q.dtype) * (q - y), "paired")
    return f, dq, g


def train_step(st, s, a, r, done, s2, w, lr, noise=None, *, actor_lr=1.0, critic_lr=10.0, tau=0.001, gamma=0.99, future=True,
               critic_rmsprop=True, decay=0.99, momentum=0.0, eps=0.1, clip=None):
    """ddpg_oracle.train_step, whole, with the critic's loss weighted by w [B] -> dict(y, q, dq, critic_grads, actor_grads)."""
    O, T = st["online"], st["target"]
    t = st["step"] + 1
    y, qt = o.targets(T, s2, r, done, gamma, future)
    fc, dq, gc = critic_grads(O, s, a, y, w)
    out = dict(y=y, qt=qt, q=fc["q"][:, 0].copy(), dq=dq, critic_grads=gc)
    for k in o.CRITIC_TRAINABLE:
        if k == o.DEAD:
            continue
        g = o.clip_by_norm(gc[k], clip) if clip else gc[k]
        if critic_rmsprop:
            o.rmsprop_step(O[k], st["slot_a"][k], st["slot_b"][k], g, critic_lr * lr, decay, momentum, eps)
        else:
            o.adam_step(O[k], st["slot_a"][k], st["slot_b"][k], g, critic_lr * lr, t)
    a_out = o.actor_forward(O, s)["out"] + (0.0 if noise is None else np.asarray(noise, np.float64)[None, :])
    g = o.action_gradient(O, s, a_out)
    _, ga = o.actor_grads(O, s, g)
    out.update(a_out=a_out, g=g, actor_grads=ga)
    for k in o.ACTOR_TRAINABLE:
        o.adam_step(O[k], st["slot_a"][k], st["slot_b"][k], ga[k], actor_lr * lr, t)
    o.soft_update(O, T, tau)
    st["step"] = t
    return out
