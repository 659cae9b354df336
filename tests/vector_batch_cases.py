"""The cases of tests/test_gpu_vector_batch.py (not collected: no test_ prefix), shared with tests/test_vector_batch_cpu.py, which
runs every case on the oracles alone and asserts what makes it worth running.

ga3c_mlp_create and ga3c_dmlp_create admit max_batch up to MAX_BATCH = 65536, and the batch size is the dimension along which
their kernels' arithmetic changes character: one thread adds a gradient element's B terms in row order (elem_grad of
csrc/ga3c_mlp.hip; sum_rows / dot_rows of csrc/ga3c_tile.hpp, in blocks of ROWS_AHEAD = 16 with a tail loop), the three loss sums
are B terms of one sign, and the tile kernels run up to 4096 workgroups of TILE = 16 rows.  SIZES: the first size past what the
older files test, a size whose remainder mod 16 is 3 (both tails), a size where a float32 chain is past the BLAS bound, and the
limit with its last tile short by one and full.

Rows.  The recipes of the older files: vector_limit_cases.params / batch (with safe_rows) at seed 100 + B for ga3c_mlp,
test_gpu_dmlp._params / _batch at seed 100 + B for ga3c_dmlp.  Neither network has ReLU units.

Heavy rows.  At 65536 rows a sum that stops one row short moves a gradient by less than its bound: no comparison sees it.  So
every size has two further batches, the same rows with ONE return multiplied by HEAVY: 'last' at row B - 1, 'tile' at the first
row of the last tile.  tests/test_vector_batch_cpu.py asserts that leaving that row (or the whole last tile) out of a sum moves
every gradient by more than two bounds.  Their oracle tensors exchange that row's term in the plain batch's (Case._swap).

Bounds.  closeness.py as it stands, e32 from the float32 oracle on the same rows; a bias of ONE element takes the larger of its
draw and closeness.e32_of_row_sum of the delta it sums.  serial_sum restates the kernels' order in numpy: float32 operands, the
products and the chain in double, rounded to float32 once.  (Until this file the chains were float32, and restated so --
g += x[r][:, None] * d[r][None, :] row by row -- they sat at up to 3.9 of these bounds at 65536 rows, against numpy's blocked
float32 matmul at 2e-7 .. 4e-7 at every size; tests/README.md keeps that table.)  The restatement's own rel_err
against float64 stays below half of every bound (the CPU file asserts it), so no tensor needs an e32 of its own, as the float32
chains did.  Nothing is taken from a kernel."""
import functools

import numpy as np

import closeness as c
import dmlp_oracle as dm
import mlp_oracle as m
import vector_limit_cases as vc

MAX_BATCH, TILE, ROWS_AHEAD = 65536, 16, 16
SIZES = [1025, 4099, 16384, 65535, 65536]
LARGE_SIZES = [4099, 65536]
BETA = vc.BETA
# The smallest power of ten for which a sum without the heavy row moves every gradient of every network below by more than two
# bounds at EVERY size, which is what tests/test_vector_batch_cpu.py asserts.  With the bounds as they stand (chains in double) the
# least over all cases is 11.5 bounds, logits_p/b of dmlp-chained at 65535 rows, row 65534; the movement is linear in HEAVY, so 100
# leaves 1.15 there.  (At 65536 rows alone 100 would do: measured with the wider bounds of the float32 chains the kernels had
# when this was chosen, its least was 3.8 bounds, logits_v/w of dmlp-fork, and 10 left 0.45.)
HEAVY = 1000.0
KINDS = ("plain", "last", "tile")

EIGHT_WIDTHS = (256, 129, 7, 33, 5, 128, 3, 1)          # test_gpu_dmlp.EIGHT
# id -> (network, S, A, layers, stack)
NETS = {"mlp-3-1": ("mlp", 3, 1, None, None), "mlp-64-32": ("mlp", 64, 32, None, None),
        "dmlp-fork": ("dmlp", 4, 2, (10, 10, 10, 10), "fork"), "dmlp-chained": ("dmlp", 4, 2, (10, 10, 10, 10), "chained"),
        "dmlp-eight": ("dmlp", 64, 32, EIGHT_WIDTHS, "chained")}
LARGE = ("mlp-64-32", "dmlp-eight")
DMLP_HEADS = {"plain": dict(use_log_softmax=False, min_policy=0.0), "log_softmax": dict(use_log_softmax=True, min_policy=0.0)}
# every (net, head, B) of the row tests
CASES = [(n, h, B) for n, spec in NETS.items() for h in (("angle",) if spec[0] == "mlp" else tuple(DMLP_HEADS))
         for B in (LARGE_SIZES if n in LARGE else SIZES)]
CASE_IDS = ["%s-%s-B%d" % t for t in CASES]
LOSSES = ("cost_p_1_agg", "cost_p_2_agg", "cost_v")


def last_tile(B):
    """The first row of the last tile of a batch of B rows."""
    return (B - 1) // TILE * TILE


def heavy_row(kind, B):
    return {"last": B - 1, "tile": last_tile(B)}[kind]


class Net:
    """One (network, shape, head): its parameters, rows, oracle and the names of what the tests compare."""

    def __init__(self, net_id, head):
        self.id, self.head = net_id, head
        self.kind, self.S, self.A, self.layers, self.stack = NETS[net_id]
        if self.kind == "mlp":
            self.params = vc.limit_params(self.S, self.A)
            self.acts = ("x", "pd1", "pd2", "pd3", "pd4", "d1", "v", "p", "z")
            self.deltas = ("dv", "dz", "dd1", "dpd4", "dpd3", "dpd2", "dpd1")
            self.grads = m.PARAM_ORDER
            self.widths = dict(x=self.S, pd1=4, pd2=256, pd3=256, pd4=100, d1=64, v=1, p=self.A, z=2 * self.A, dv=1, dz=2 * self.A,
                               dd1=64, dpd4=100, dpd3=256, dpd2=256, dpd1=4)
            self.first_delta = "dpd1"
        else:
            from test_gpu_dmlp import _params
            self.params = _params(self.S, self.A, self.layers, self.stack)
            self.kw = DMLP_HEADS[head]
            nl = len(self.layers)
            self.live = list(range(1, nl + 1)) if self.stack == "chained" else [nl]
            self.acts = ("x",) + tuple("h%d" % i for i in self.live) + ("v", "p", "z")
            self.deltas = ("dv", "dz") + tuple("dh%d" % i for i in reversed(self.live))
            dead = dm.dead_params(self.layers, self.stack)
            self.dead = dead
            self.grads = tuple(k for k in dm.param_order(self.layers) if k not in dead)
            self.widths = dict(x=self.S, v=1, p=self.A, z=self.A, dv=1, dz=self.A)
            for i in self.live:
                self.widths["h%d" % i] = self.widths["dh%d" % i] = self.layers[i - 1]
            self.first_delta = "dh%d" % self.live[0]
        self.flat = (m if self.kind == "mlp" else dm).flat

    def batch(self, B, seed=None):
        seed = 100 + B if seed is None else seed
        if self.kind == "mlp":
            return vc.batch(self.params, B, self.S, self.A, seed)
        from test_gpu_dmlp import _batch
        return _batch(B, self.S, self.A, seed)

    def grads_of(self, params, x, y, a):
        """The oracle in the dtype of `params` -> (losses, every compared tensor by name)."""
        dt = next(iter(params.values())).dtype
        x, y, a = (np.asarray(t, dt) for t in (x, y, a))
        with np.errstate(over="ignore"):
            if self.kind == "mlp":
                f = m.forward(params, x)
                losses, g = m.loss_and_grads(params, x, y, a, BETA)
                f["p"] = f["o"]
            else:
                f = dm.forward(params, x, self.stack, **self.kw)
                losses, g = dm.loss_and_grads(params, x, y, a, BETA, stack=self.stack, **self.kw)
        t = {k: np.asarray(f[k]) for k in self.acts}
        t.update({k: np.asarray(g[k]) for k in self.deltas + self.grads})
        return losses, t

    def train_step(self, ref, ms, mom, x, y, a, lr, momentum=0.0, clip=None):
        """One production step of the float64 oracle, in place -> its gradients."""
        if self.kind == "mlp":
            _, g = m.loss_and_grads(ref, *vc.f64(x, y, a), BETA)
            m.rmsprop_update(ref, ms, g, lr, momentum=momentum, mom=mom, clip=clip)
            return g
        return dm.train_step(ref, ms, mom, *vc.f64(x, y, a), lr, BETA, stack=self.stack, momentum=momentum, clip=clip, **self.kw)[1]

    def sources(self, t):
        """[(weight, bias, the rows' input, the rows' delta)] of every live layer, from the tensors `t`."""
        A = self.A
        if self.kind == "mlp":
            ins = ("x", "pd1", "pd2", "pd3", "pd4")
            outs = ("dpd1", "dpd2", "dpd3", "dpd4", "dd1")
            src = [(name + "/w", name + "/b", t[i], t[d]) for (name, _, _), i, d in zip(m.TRUNK, ins, outs)]
            for name, d in zip(m.HEADS, (t["dv"][:, None], t["dz"][:, :A], t["dz"][:, A:])):
                src.append((name + "/w", name + "/b", t["d1"], d))
            return src
        src = []
        for i in self.live:
            name = "dense1_%d_p" % i
            src.append((name + "/w", name + "/b", t["h%d" % (i - 1)] if self.stack == "chained" and i > 1 else t["x"], t["dh%d" % i]))
        hl = t["h%d" % len(self.layers)]
        return src + [("logits_v/w", "logits_v/b", hl, t["dv"][:, None]), ("logits_p/w", "logits_p/b", hl, t["dz"])]

    def blas_e32(self, name, t32, t64):
        """closeness's e32 of one delta or gradient; a bias of ONE element takes the larger of its draw and e32_of_row_sum of the
        delta it sums."""
        e = c.rel_err(t32[name], t64[name])
        if name.endswith("/b") and np.size(t64[name]) == 1:
            d32, d64 = (next(d for _, bn, _, d in self.sources(t) if bn == name) for t in (t32, t64))
            e = max(e, c.e32_of_row_sum(d32, d64))
        return e


@functools.lru_cache(maxsize=None)
def net(net_id, head):
    return Net(net_id, head)


def serial_sum(x, d):
    """The kernels' chains on the rows' inputs x and deltas d (float32): products and sums in double, rounded to d's dtype once
    -> (weight gradient, bias gradient).  A chain in double is off by 1e-16 x B whatever its order, far below that one rounding,
    so the row order itself is not restated."""
    x64, d64 = np.asarray(x, np.float64), np.asarray(d, np.float64)
    return (x64.T @ d64).astype(d.dtype), d64.sum(axis=0).astype(d.dtype)


class Case:
    """One (net, head, B): the rows, and per kind of batch (plain, heavy 'last', heavy 'tile') the returns y, the oracle's tensors
    in float64 (want) and float32 (w32), its losses, e32 of every delta and gradient, and the restatement of the kernels' chains
    for every gradient: serial[kind][name] = (its rel_err against float64, that as a share of the bound)."""

    def __init__(self, net_id, head, B):
        self.net, self.B = net(net_id, head), B
        n = self.net
        self.x, y, self.a = n.batch(B)
        self.y, self.losses, self.want, self.w32, self.e32, self.serial = {}, {}, {}, {}, {}, {}
        p32 = vc.f32_params(n.params)
        plain = n.grads_of(n.params, self.x, y, self.a), n.grads_of(p32, self.x, y, self.a)
        self.y["plain"] = y
        for kind in KINDS:
            if kind == "plain":
                (self.losses[kind], self.want[kind]), (_, self.w32[kind]) = plain
            else:
                yk = y.copy()
                yk[heavy_row(kind, B)] *= np.float32(HEAVY)
                self.y[kind] = yk
                self.losses[kind], self.want[kind] = self._swap(n.params, plain[0], heavy_row(kind, B), yk)
                _, self.w32[kind] = self._swap(p32, plain[1], heavy_row(kind, B), yk)
            w, w32 = self.want[kind], self.w32[kind]
            self.e32[kind] = {k: n.blas_e32(k, w32, w) for k in n.deltas + n.grads}
            self.serial[kind] = {}
            for wn, bn, xin, d in n.sources(w32):
                g, b = serial_sum(xin, d)
                assert g.dtype == np.float32 and b.dtype == np.float32, wn
                for k, got in ((wn, g), (bn, b)):
                    err = c.rel_err(got, w[k])
                    self.serial[kind][k] = (err, err / self.bound(kind, k))

    def _swap(self, params, plain, r, yk):
        """The oracle on the batch whose row r has the return yk[r], in the dtype of `params`, from its run on the plain batch:
        a row's outputs and deltas depend on no other row, and every gradient and loss is a sum over the rows, so row r's deltas
        are replaced and its term of every sum (the oracle on that row alone) is exchanged."""
        n, rows = self.net, slice(r, r + 1)
        losses, t = plain
        l0, t0 = n.grads_of(params, self.x[rows], self.y["plain"][rows], self.a[rows])
        l1, t1 = n.grads_of(params, self.x[rows], yk[rows], self.a[rows])
        out = dict(t)
        for k in n.deltas:
            out[k] = t[k].copy()
            out[k][r] = t1[k][0]
        for k in n.grads:
            out[k] = t[k] + (t1[k] - t0[k])
        return {k: losses[k] + (l1[k] - l0[k]) for k in LOSSES}, out

    def bound(self, kind, name):
        return c.bound(self.e32[kind][name])

    def rows_term(self, kind, rows):
        """What a sum that leaves `rows` out is short of, per gradient: the float64 oracle on those rows alone."""
        n = self.net
        return n.grads_of(n.params, self.x[rows], self.y[kind][rows], self.a[rows])[1]


@functools.lru_cache(maxsize=None)
def case(net_id, head, B):
    return Case(net_id, head, B)


# ---- two production steps
STEP_SIZES = [4099, 65536]
STEP_NETS = [("mlp-3-1", "angle"), ("dmlp-chained", "plain")]
STEP_WAYS = {"plain": dict(), "momentum": dict(momentum=0.9), "clip": dict(clip=True)}
STEP_LR = 1e-3                                    # test_gpu_vector_limits', test_gpu_dmlp's
# ||g|| / n of every variable is far above this at 4099 rows and more (asserted from the oracle's gradients at every step)
STEP_CLIP = 1e-4
PERMUTATION_SEED = 65536
SAME_ROWS = (0, 15, 16, 1024, 65520, 65535)


@functools.lru_cache(maxsize=None)
def step_batch(net_id, head, B, step):
    """The rows of step `step` of the two-step tests (seed 7 + step, as the older files), shared by their ways."""
    return net(net_id, head).batch(B, seed=7 + step)


def permutation(B):
    return np.random.Generator(np.random.PCG64(PERMUTATION_SEED)).permutation(B)


# ---- the device actors at the row limit: 16 environments per thread of the 1024-thread scan, N x (TIME_MAX + 1) = 65536 rows
# game -> (net, head, N, TIME_MAX).  CartPole at the issue's N = 4096, TIME_MAX = 15 ends episodes by itself before the first cut
# (17 steps from a pole at +-0.05 rad), so that case would not lay out N x T1 rows; the issue allows moving N and TIME_MAX at a
# constant row count, and within 5 steps no pole falls (tests/test_vector_batch_cpu.py asserts both oracles' row counts).
ACTOR_CASES = {"cartpole": ("dmlp-fork", "plain", 16384, 3), "pendulum": ("mlp-3-1", "angle", 16384, 3)}
ACTOR_GAMMA, ACTOR_SEED, ACTOR_TRAIN_SEED = 0.99, 65543, 65551


def actors_oracle(game, seed=ACTOR_SEED):
    """-> (the actors' oracle of the case, N, TIME_MAX)."""
    import device_agents_oracle as dao
    import device_pendulum_oracle as dpo
    _, _, n, time_max = ACTOR_CASES[game]
    make = dao.Actors if game == "cartpole" else dpo.PendulumActors
    return make(n, seed, time_max, ACTOR_GAMMA), n, time_max
