"""The cases of tests/test_gpu_ddpg_batch.py and the choice of their rows (not collected: no test_ prefix), shared with
tests/test_ddpg_batch_cpu.py, which runs every case on the oracles alone and asserts what makes it worth running.

The DDPG handle admits max_batch up to MAX_B = 4096, and three loops of csrc/ga3c_ddpg.hip take a second trip only past a
thread count: the sums over y of critic_step and ddpg_popart_kernel stride by THREADS = 448, the draws and the weight maximum of
per_sample_kernel and the rows of per_update_kernel by PER_THREADS = 1024.  SIZES holds both sides of each and the limit.

Rows.  test_gpu_ddpg._select's rule and its cap of 20 rounds: 2 B candidates, the first B whose relu units all keep 1e-4 away
from zero in the oracle, re-checked where step 4 evaluates the critic AFTER its step.  That step depends on the whole batch, and
at the critic's usual rate (10 x 3e-4) replacing the 1 - 2 % of rows that fail moves it by more than the band: from 1025 rows
on the choice does not settle.  As tests/sac_cases.py, the cases keep the rule and make the movement small instead:
  * the single-step cases, which compare rows and gradients and no weight after a step, run at ROWS_LR = 3e-6;
  * the two-step cases, which hold weights and slots to 1e-5, run at LR = 3e-4 with Config.critic_lr = 1 (STEPS_CRITIC_LR).

Bounds.  closeness.py as it stands, e32 from the float32 oracle on the same rows; the one-element critic_output/b takes the
larger of its draw and closeness.e32_of_row_sum of dq.  wgrad_element sums a gradient element over the B rows in row order in
float32, at 4096 rows the longest chain of the project, and numpy's float32 matmul (blocked, pairwise) is a far better order
than that.  serial_sum restates the kernel's order in numpy float32; where its own rel_err against float64 is above half of
the bound a tensor would be held to, that tensor's e32 at that size is the restatement's (RowCase.e32, RowCase.restated)."""
import functools

import numpy as np

import closeness as c
import ddpg_oracle as o
import device_agents_oracle as dao
import per_oracle as per
from test_gpu_ddpg import LR, _candidates, _cfg_kw

ROWS_LR = 3e-6
STEPS_CRITIC_LR = 1.0
THREADS, PER_THREADS, MAX_B = 448, 1024, 4096
SIZES = [448, 449, 1024, 1025, 4096]
STRIDE_ROWS = (THREADS, PER_THREADS)            # the first row past each stride
SHAPE, LARGE = (7, 3), (64, 32)
FORMS = ("fork", "paired")
ROW_CASES = [SHAPE + (B,) for B in SIZES] + [LARGE + (MAX_B,)]
STEP_SIZES = [449, 1025, 4096]
STEP_WAYS = {"rmsprop": dict(), "adam": dict(RMSPROP=False), "clip-momentum": dict(USE_GRAD_CLIP=True, RMSPROP_MOMENTUM=0.9)}
# A row whose q happens to lie at the mean of y has no dq in the fork form, and a sum short of that row is short of nothing.  At
# (64, 32) the base 7000 put such a row at place 448; 7100 is the first of 7000, 7100, .. at which a sum short of row B - 1, 448 or
# 1024 moves every gradient of both nets by more than two bounds in both loss forms (tests/test_ddpg_batch_cpu.py asserts it).
ROW_SEEDS = {LARGE: 7100}
CAPACITY = 2 * MAX_B                            # the shared handles' ring: two batches of the limit


def f64(batch):
    return tuple(np.asarray(t, np.float64) for t in batch)


def f32(P):
    return {k: v.astype(np.float32) for k, v in P.items()}


def copy_state(st):
    return dict(st, online={k: v.copy() for k, v in st["online"].items()}, target={k: v.copy() for k, v in st["target"].items()},
                slot_a={k: v.copy() for k, v in st["slot_a"].items()}, slot_b={k: v.copy() for k, v in st["slot_b"].items()})


def select(st, cand, B, noise, lr, **kw):
    """test_gpu_ddpg._select at the rate `lr` (and kw's critic_lr) -> (the B chosen rows, rounds taken)."""
    s, a, r, done, s2 = cand
    ok = o.relu_margin(st["online"], st["target"], s, a, s2) > 1e-4
    nz = 0.0 if noise is None else np.asarray(noise, np.float64)[None, :]
    for rounds in range(1, 21):
        keep = np.flatnonzero(ok)[:B]
        assert keep.size == B, "only %d of %d candidate rows qualify" % (keep.size, ok.size)
        trial = copy_state(st)
        rows = tuple(np.asarray(t[keep], np.float64) for t in cand)
        o.train_step(trial, *rows, lr, None, stop_after=3, **kw)
        a_out = o.actor_forward(trial["online"], rows[0])["out"] + nz
        bad = np.abs(o.critic_forward(trial["online"], rows[0], a_out)["t"]).min(axis=1) <= 1e-4
        if not bad.any():
            return tuple(t[keep] for t in cand), rounds
        ok[keep[bad]] = False
    raise AssertionError("the choice of rows did not settle")


# ---- steps 1 - 4: every row and gradient

# variable -> (the rows' input or None, the rows' multiplier or None, the rows' delta): GradSrc of the engine, by the oracle's names
def _sources(P, f, d_out, net):
    """The per-row operands of every gradient of one net, from the oracle's forward / backward dict f, in f's dtype."""
    if net == "critic":
        dh1 = f["dn1"] * (P["critic_norm1/gamma"] * f["rs1"])
        return {"critic_output/W": (f["c2"], None, d_out[:, None]), "critic_output/b": (None, None, d_out[:, None]),
                "critic_fc2/W": (f["c1"], None, f["dt"]), "critic_norm2/W": (f["a"], None, f["dt"]),
                "critic_norm2/b": (None, None, f["dt"]), "critic_norm1/beta": (None, None, f["dn1"]),
                "critic_norm1/gamma": (None, f["xh1"], f["dn1"]), "critic_fc1/W": (f["x"], None, dh1),
                "critic_fc1/b": (None, None, dh1)}
    dh2 = f["dn2"] * (P["actor_norm2/gamma"] * f["rs2"])
    dh1 = f["dn1"] * (P["actor_norm1/gamma"] * f["rs1"])
    return {"actor_output/W": (f["a2"], None, f["do"]), "actor_output/b": (None, None, f["do"]),
            "actor_norm2/beta": (None, None, f["dn2"]), "actor_norm2/gamma": (None, f["xh2"], f["dn2"]),
            "actor_fc2/W": (f["a1"], None, dh2), "actor_fc2/b": (None, None, dh2), "actor_norm1/beta": (None, None, f["dn1"]),
            "actor_norm1/gamma": (None, f["xh1"], f["dn1"]), "actor_fc1/W": (f["x"], None, dh1), "actor_fc1/b": (None, None, dh1)}


def serial_sum(x, mul, d):
    """wgrad_element's order in d's dtype: a loop over the rows, g += x[r][:, None] * d[r][None, :] (mul[r] * d[r]; d[r])."""
    g = np.zeros((x.shape[1], d.shape[1]) if x is not None else d.shape[1], d.dtype)
    for r in range(d.shape[0]):
        if x is not None:
            g += x[r][:, None] * d[r][None, :]
        elif mul is not None:
            g += mul[r] * d[r]
        else:
            g += d[r]
    return g


def row_term(src, r):
    """Row r's term of one gradient (what a sum that leaves the row out is short of)."""
    x, mul, d = src
    return x[r][:, None] * d[r][None, :] if x is not None else (mul[r] * d[r] if mul is not None else d[r])


def tensors(out):
    """The deltas and gradients that closeness.py holds (test_gpu_ddpg's test_backward_tensors_relative...)."""
    fc, fa = out["critic_fwd"], out["actor_fwd"]
    t = {"dq": out["dq"], "c_dt": fc["dt"], "c_dn1": fc["dn1"], "g": out["g"], "do": fa["do"], "a_dn2": fa["dn2"], "a_dn1": fa["dn1"]}
    t.update({"grad " + k: out["critic_grads"][k] for k in o.CRITIC_TRAINABLE if k != o.DEAD})
    t.update({"grad " + k: out["actor_grads"][k] for k in o.ACTOR_TRAINABLE})
    return t


class RowCase:
    """One (S, A, B, loss form): weights, rows, the oracle's steps 1 - 4 in float64 (out, want) and float32 (w32), e32 of every
    compared tensor, and -- restate=True -- the serial restatement of every gradient with its rel_err / bound."""

    def __init__(self, S, A, B, form, restate=True, seed=None):
        self.S, self.A, self.B, self.form = S, A, B, form
        self.noise = np.linspace(-0.2, 0.3, A).astype(np.float32)
        rng = np.random.Generator(np.random.PCG64(ROW_SEEDS.get((S, A), 7000) + B + S if seed is None else seed))
        self.online, self.target = o.random_params(S, A, rng, stats=True), o.random_params(S, A, rng, stats=True)
        self.batch, self.rounds = select(o.new_state(self.online, self.target), _candidates(S, A, 2 * B, rng), B, self.noise,
                                         ROWS_LR, form=form)
        self.st = o.new_state(self.online, self.target)
        self.out = o.train_step(self.st, *f64(self.batch), ROWS_LR, self.noise.astype(np.float64), stop_after=4, form=form)
        st32 = o.new_state(f32(self.online), f32(self.target))
        self.out32 = o.train_step(st32, *self.batch, ROWS_LR, self.noise, stop_after=4, form=form)
        self.want, self.w32 = tensors(self.out), tensors(self.out32)
        self.blas = {k: c.rel_err(self.w32[k], v) for k, v in self.want.items()}
        self.blas["grad critic_output/b"] = max(self.blas["grad critic_output/b"], c.e32_of_row_sum(self.w32["dq"], self.want["dq"]))
        self.e32 = dict(self.blas)
        self.serial, self.restated = {}, {}
        if restate:
            # the critic's sources at the weights its gradient was taken at (st holds them after step 3), the actor's at st's
            src32 = dict(_sources(f32(self.online), self.out32["critic_fwd"], self.out32["dq"], "critic"),
                         **_sources(st32["online"], self.out32["actor_fwd"], None, "actor"))
            for k, s in src32.items():
                g = serial_sum(*s)
                assert g.dtype == np.float32, k
                err = c.rel_err(g, self.want["grad " + k])
                self.serial[k] = (err, err / c.bound(self.blas["grad " + k]))
                if err > 0.5 * c.bound(self.blas["grad " + k]):
                    self.restated[k] = (self.blas["grad " + k], err)
                    self.e32["grad " + k] = max(err, self.blas["grad " + k])

    def sources(self):
        """The float64 per-row operands of every gradient of both nets."""
        return dict(_sources(self.online, self.out["critic_fwd"], self.out["dq"], "critic"),
                    **_sources(self.st["online"], self.out["actor_fwd"], None, "actor"))

    def bound(self, name):
        return c.bound(self.e32[name])


@functools.lru_cache(maxsize=None)
def row_case(S, A, B, form, restate=True):
    return RowCase(S, A, B, form, restate)


# ---- two full steps

class StepCase:
    """Two steps of train() at B rows, (7, 3), LR with critic_lr = 1: the rows of each step (chosen on the oracle's state as it
    then stood), what each step returned and the oracle's state after both."""

    def __init__(self, B, way, steps=2):
        S, A = SHAPE
        self.B, self.cfg = B, STEP_WAYS[way]
        self.kw = dict(_cfg_kw(self.cfg), critic_lr=STEPS_CRITIC_LR)
        self.noise = np.full(A, 0.05, np.float32)
        rng = np.random.Generator(np.random.PCG64(8000 + B))
        self.online, self.target = o.random_params(S, A, rng), o.random_params(S, A, rng)
        self.st = o.new_state(self.online, self.target, critic_rmsprop=self.cfg.get("RMSPROP", True))
        self.batches, self.outs, self.rounds, self.after_first = [], [], [], None
        for i in range(steps):
            b, rounds = select(self.st, _candidates(S, A, 2 * B, rng), B, self.noise, LR, **self.kw)
            self.batches.append(b)
            self.rounds.append(rounds)
            self.outs.append(o.train_step(self.st, *f64(b), LR, self.noise.astype(np.float64), **self.kw))
            if i == 0:
                self.after_first = {k: v.copy() for k, v in self.st["online"].items()}


@functools.lru_cache(maxsize=None)
def step_case(B, way):
    return StepCase(B, way)


# ---- prioritised replay

PER_SHAPE = (3, 1)
ALPHA, EPS, PER_SEED = 0.6, 0.01, 12345         # test_gpu_prioritized_replay's
PER_SIZES = [1024, 1025, 4096]
HEAVY_SLOT = 700
TAIL = 200


def random_priorities(capacity, size, rng):
    """test_gpu_prioritized_replay._random_priorities."""
    pa = np.zeros(capacity, np.float32)
    pa[:size] = rng.uniform(0.01, 2, size).astype(np.float32) ** np.float32(0.6)
    return pa


def heavy_priorities(size):
    """test_heavy_tail_duplicates...'s ring: every slot at 1e-3 but one at 50."""
    pa = np.full(size, 1e-3, np.float32)
    pa[HEAVY_SLOT] = 50.0
    return pa


@functools.lru_cache(maxsize=None)
def ring(kind):
    """-> (capacity, pa f32 [capacity], max_pa): 'tail' (below), 'near' 5000 rows (B close to size: many strata inside one chunk), 'million'
    1 048 576 rows, 'heavy' 2049 rows, 'heavy-wide' the same on 4100 rows (train_prioritized wants MORE rows than a batch)."""
    if kind == "near":
        return 5000, random_priorities(5000, 5000, np.random.default_rng(5000)), 2.0
    if kind == "tail":
        # the 5000 rows again, but only the LAST row of a draw of 1025 reaches the batch's largest weight: the last TAIL slots share
        # a mass of (1 - u / 2) strata, u the last row's uniform, at a priority below every other slot's, so row 1024 -- the second
        # row of per_sample_kernel's thread 0 -- lands among them and row 1023 before them
        size, B = 5000, PER_THREADS + 1
        pa = random_priorities(size, size, np.random.default_rng(5001))
        f = 1.0 - float(dao.uniform(PER_SEED, 0, np.array([B - 1]))[0]) / 2.0
        rest = float(np.sum(pa[:size - TAIL], dtype=np.float64))
        pa[size - TAIL:] = np.float32(f * rest / (B - f) / TAIL)
        return size, pa, 2.0
    if kind == "million":
        return per.MAX_CAPACITY, random_priorities(per.MAX_CAPACITY, per.MAX_CAPACITY, np.random.default_rng(7)), 2.0
    size = {"heavy": 2049, "heavy-wide": 4100}[kind]
    return size, heavy_priorities(size), 50.0


@functools.lru_cache(maxsize=None)
def draw(kind, B, number):
    """per_oracle.draw of sample `number` on the ring -> (slots, total_pa, clamped)."""
    size, pa, _ = ring(kind)
    return per.draw(pa, size, B, PER_SEED, number)


# the draws of test_gpu_ddpg_batch.py: ring -> [(B, sample number)], the numbers in the order one handle takes them
DRAWS = {"tail": [(1025, 0)], "near": [(1024, 0), (1025, 1), (4096, 2)], "million": [(4096, 0)], "heavy": [(1024, 0), (1025, 1), (4096, 2)]}
UPDATES = [("heavy", 1025), ("heavy-wide", 4096)]
WEIGHTED = dict(n=2048, B=1025, beta=0.4, seed=9100)


@functools.lru_cache(maxsize=None)
def weighted_case():
    """The weighted step at 1025 rows: priorities, the oracle's draw and weights, and a ring of 2048 rows chosen by
    test_gpu_prioritized_replay._ring_for_batch at LR with critic_lr = 1 -> (pa, slots, w, noise, online, target, rows)."""
    from test_gpu_prioritized_replay import _ring_for_batch
    n, B = WEIGHTED["n"], WEIGHTED["B"]
    noise = np.full(PER_SHAPE[1], 0.05, np.float32)
    pa = random_priorities(n, n, np.random.default_rng(5))
    slots, w = per.sample(pa, n, B, PER_SEED, 0, WEIGHTED["beta"])
    online, target, rows = _ring_for_batch(n, WEIGHTED["seed"], slots, w, noise, critic_lr=STEPS_CRITIC_LR)
    return pa, slots, w, noise, online, target, rows


# ---- the uniform draw of the device actors

ACTORS_N, ACTORS_PREFILL, DRAW_SEED = 64, 5000, 24680
ACTORS_SIZES = [1025, 4096]


# ---- the options at 449 and 4096 rows, (7, 3): one step each, every row and gradient, at ROWS_LR

OPTION_SIZES = [449, 4096]
POPART_BETA, POPART_MU, POPART_NU, POPART_OFFSET = 0.5, -97.0, 9500.0, -100.0     # test_gpu_popart's "near-100" statistics
TWIN = dict(policy_delay=1, sigma=1.0, noise_clip=0.3)                            # the clip applies to most draws
TWIN_SEED = 12345                                                                 # test_gpu_td3.SEED
ATOMS, VMIN, VMAX = 51, -3.0, 1.0                                                 # test_gpu_dist's support


def _noise(A):
    return np.linspace(-0.2, 0.3, A).astype(np.float32)


@functools.lru_cache(maxsize=None)
def popart_case(B):
    """y = r exactly (no future reward), r = -100 + 0.09 u as test_gpu_popart._kernel_case, from statistics near -100; the rows by
    test_gpu_popart._select with the step at ROWS_LR -> (online, target, batch, noise, kw of popart_oracle.train_step)."""
    import popart_oracle as po
    from test_gpu_popart import _select
    S, A = SHAPE
    rng = np.random.Generator(np.random.PCG64(8500 + B))
    online, target = o.random_params(S, A, rng, stats=True), o.random_params(S, A, rng, stats=True)
    s, a, r, done, s2 = _candidates(S, A, 2 * B, rng)
    r = (np.float32(POPART_OFFSET) + np.float32(0.09) * r).astype(np.float32)
    noise = _noise(A)
    kw = dict(beta=POPART_BETA, future=False)
    st = po.new_state(online, target, mu=float(np.float32(POPART_MU)), nu=float(np.float32(POPART_NU)))
    batch = _select(st, (s, a, r, done, s2), B,
                    lambda trial, rows: po.train_step(trial, *rows, ROWS_LR, noise.astype(np.float64), stop_after=4, **kw))
    return online, target, batch, noise, kw


def select_twin(st, cand, B, noise, lr, tw, **kw):
    """test_gpu_td3._select at the rate `lr` -> (rows, candidates tried): 4 B candidates, a row that fails td3_oracle.relu_margin
    under the smoothing noise of its place, or the second layer of critic 1 after step 3, gives its place to the next one."""
    import td3_oracle as t3
    n, A = cand[1].shape
    assert n == 4 * B
    t = st["step"] + 1
    eps = t3.smoothing_noise(TWIN_SEED, t, B, A, tw["sigma"], tw["noise_clip"])
    nz = np.asarray(noise, np.float64)[None, :]
    place, tried = np.full(B, -1), 0
    for _ in range(60):
        need = np.flatnonzero(place < 0)
        assert tried + need.size <= n, "only %d of %d candidate rows qualify" % (B - need.size, n)
        place[need] = np.arange(tried, tried + need.size)
        tried += need.size
        rows = f64(tuple(t_[place] for t_ in cand))
        bad = t3.relu_margin(st["online"], st["target"], rows[0], rows[1], rows[4], eps) <= 1e-4
        if not bad.any() and t % tw["policy_delay"] == 0:
            trial = copy_state(st)
            t3.train_step(trial, *rows, lr, None, eps=eps, stop_after=3, **tw, **kw)
            a_out = o.actor_forward(trial["online"], rows[0])["out"] + nz
            bad = np.abs(o.critic_forward(trial["online"], rows[0], a_out)["t"]).min(axis=1) <= 1e-4
        if not bad.any():
            return tuple(t_[place] for t_ in cand), tried
        place[bad] = -1
    raise AssertionError("the choice of rows did not settle")


@functools.lru_cache(maxsize=None)
def twin_case(B):
    import td3_oracle as t3
    S, A = SHAPE
    rng = np.random.Generator(np.random.PCG64(8600 + B))
    online, target = t3.random_params(S, A, rng, stats=True), t3.random_params(S, A, rng, stats=True)
    noise = _noise(A)
    batch, tried = select_twin(t3.new_state(online, target), _candidates(S, A, 4 * B, rng), B, noise, ROWS_LR, TWIN)
    return online, target, batch, noise, tried


def dist_candidates(S, A, n, N, rng):
    """test_gpu_dist._dcandidates: rewards over (-5, 3), every fifth row done with its reward on an atom."""
    import dist_oracle as d4
    s, a, _, done, s2 = _candidates(S, A, n, rng)
    r = rng.uniform(-5.0, 3.0, n).astype(np.float32)
    on = np.arange(n) % 5 == 0
    done[on] = 1.0
    r[on] = d4.support(N, VMIN, VMAX)[0][rng.integers(0, N, int(on.sum()))].astype(np.float32)
    return s, a, r, done, s2


def select_dist(st, cand, B, noise, lr, **kw):
    """test_gpu_dist._dselect at the rate `lr` -> (rows, rounds)."""
    import dist_oracle as d4
    s, a, r, done, s2 = cand
    ok = d4.relu_margin(st["online"], st["target"], s, a, s2) > 1e-4
    nz = np.asarray(noise, np.float64)[None, :]
    for rounds in range(1, 21):
        keep = np.flatnonzero(ok)[:B]
        assert keep.size == B, "only %d of %d candidate rows qualify" % (keep.size, ok.size)
        trial = copy_state(st)
        rows = tuple(np.asarray(t[keep], np.float64) for t in cand)
        d4.train_step(trial, *rows, lr, None, stop_after=3, **kw)
        a_out = o.actor_forward(trial["online"], rows[0])["out"] + nz
        bad = np.abs(o.critic_forward(trial["online"], rows[0], a_out)["t"]).min(axis=1) <= 1e-4
        if not bad.any():
            return tuple(t[keep] for t in cand), rounds
        ok[keep[bad]] = False
    raise AssertionError("the choice of rows did not settle")


DIST_KW = dict(atoms=ATOMS, vmin=VMIN, vmax=VMAX)


@functools.lru_cache(maxsize=None)
def dist_case(B):
    import dist_oracle as d4
    S, A = SHAPE
    rng = np.random.Generator(np.random.PCG64(8700 + B))
    online, target = d4.random_params(S, A, ATOMS, rng, stats=True), d4.random_params(S, A, ATOMS, rng, stats=True)
    noise = _noise(A)
    batch, rounds = select_dist(d4.new_state(online, target), dist_candidates(S, A, 4 * B, ATOMS, rng), B, noise, ROWS_LR, **DIST_KW)
    return online, target, batch, noise, rounds


@functools.lru_cache(maxsize=None)
def soft_case(B):
    """sac_cases.every_row_case at (7, 3): its rule, its seeds, its ROWS_LR -> (online, target, batch, tried)."""
    import sac_cases as sc
    assert sc.ROWS_LR == ROWS_LR
    return sc.every_row_case(SHAPE[0], SHAPE[1], B)
