"""The cases of tests/test_backward_cases_cpu.py and tests/test_gpu_backward_seams.py (not collected: no test_ prefix): the
image net's backward pass and production step above 160 rows, on both sides of every change of their launch rules.  Both
files build their cases here, so the conditions the CPU file asserts are the conditions of the rows the GPU file runs.

    bwd_path(B)               the launch rules restated: conv backward form, slab counts, loop trips, chunk rows, gather form
    regime(B)                 bwd_path without the trip counts and the sizes that follow B row by row
    SIZES                     both sides of every change of regime between 161 and 1025 rows, one past every 128-row chunk
    entries()                 forward_cases.pool()'s 67 states, a return and a one-hot action bound to each, three heavy ones behind
    PoolSide                  the oracle per ENTRY (float64, float32 throughout), composed into the tensors of a batch
    index(B), index_with(..)  forward_cases.index(B) with a last row that differs from the rows 128 k in front; entry e at a given row

Why a pool.  A materialised closeness.OracleCase costs a second at 257 rows and four at 1025.  But every tensor of the backward
pass is a per-row tensor (dz, dv, dd1, dn2, dn1) or a sum over the rows of per-row terms (the ten gradients, the loss sums),
and a row's terms depend on its state, return and action alone.  So the oracle runs once per entry -- 70 one-row calls of
o.loss_and_grads on a shared forward pass -- and a batch of any size is composed:

    deltas           the entries' rows gathered by the batch's index
    dense1/w         n2[idx].T @ dd1[idx]
    other variables  the count-weighted sum of the entries' gradients
    loss sums        the count-weighted sum of the entries' terms

The float32 side, from which e32 comes, SUMS B float32 terms in float32 (gathered rows, `sum(axis=0, dtype=float32)`, a
float32 matmul for dense1/w): multiplying by the counts would round once where a batch rounds B times and understate e32.

Heavy entries (|y| = 100 against U(-1, 1)) are entries 67 .. 69, on three of the pool's states: index(B) never draws them, so
the plain batches are not dominated by them (a heavy row hides every other row's error behind its own hundredfold terms);
index_with places one at the row a test aims at.  No case or condition here touches a kernel."""
import collections
import functools

import numpy as np

import closeness as c
import forward_cases as fc
import ga3c_oracle as o

A = fc.A
BETA = 0.01
R = fc.R
HEAVY = (67, 68, 69)                   # entries behind the pool's own
HEAVY_STATES = (3, 29, 51)             # ... on these random states of the pool
HEAVY_Y = 100.0
ENTRY_SEED = 8100
MAX_BATCH = 1025
SIZES = (161, 176, 177, 192, 193, 255, 256, 257, 384, 385, 512, 513, 1024, 1025)
ONE_PAST = (193, 257, 385, 513, 1025)  # one row past a boundary: the last row is alone in its pass
WIDE = (("disc", 64), ("cont", 32), ("dual", 64))
WIDE_SIZES = (257, 513)
HEAVY_ROWS = {257: (0, 127, 255, 256), 385: (0, 383, 384), 513: (0, 511, 512), 1025: (0, 1023, 1024)}
LAST_ROW_SIZES = (257, 513, 1025)
GATHER_SIZES = (192, 193, 257)
VARS = tuple(k for k in o.PARAM_ORDER if k != "dense1/w")       # composed from per-entry gradients; dense1/w from n2 and dd1
LOSSES = ("cost_p_1_agg", "cost_p_2_agg", "cost_v")


# ---------------------------------------------------------------- the launch rules, restated
CONV_BWD_MIN_B, CONV_BWD_MAX_B = 97, 128      # ga3c_engine.hip:254
DW_PAIR_MAX_B = 256                           # ga3c_engine.hip:256
D1B_ROWS, D1B_TAIL_ROWS = 128, 5              # ga3c_kernels.hpp:1676, 1685
GATHER_ARGS_MAX_B = 192                       # ga3c_engine.hip:1147 (a literal there)
C2DX_WD_BLOCKS = fc.KSTEPS_DENSE // 2         # ga3c_kernels.hpp:2351

BwdPath = collections.namedtuple("BwdPath", "forward conv nch1 nch2 c2dw_passes c1dw_units chunks last_rows tail "
                                            "wide_w_passes wide_b_passes loss_sum_passes gather defer_wd c2dx_grid")
# the fields that count trips of a loop whose body does not change, and those that follow B row by row
LOOP_FIELDS = ("c2dw_passes", "c1dw_units", "chunks", "wide_w_passes", "wide_b_passes", "loss_sum_passes")
PER_ROW_FIELDS = ("nch2", "last_rows", "c2dx_grid")


def _ceil(n, d):
    return (n + d - 1) // d


def conv1_dw_blocks(bsz):
    """ga3c_engine.hip:580-588."""
    units, n = bsz * 7, 512
    if bsz <= 256:
        one_round = 768 - 4 * bsz
        n = one_round if 5 * one_round >= units else 256
    return min(units, n)


def bwd_path(bsz):
    """The backward pass of a train step (or compute_grads) of bsz rows on one GPU, as launch_backward lays it out."""
    fused = CONV_BWD_MIN_B <= bsz <= CONV_BWD_MAX_B                          # ga3c_engine.hip:595 (slab_geom)
    conv = "fused" if fused else ("pair" if bsz <= DW_PAIR_MAX_B else "split")      # ga3c_engine.hip:739-747
    nch1 = 2 * bsz if fused else conv1_dw_blocks(bsz)                        # ga3c_engine.hip:595-596
    nch2 = 2 * bsz if fused else (bsz if bsz < 256 else 256)
    c2dw_passes = 1 if fused else _ceil(bsz, nch2)                           # ga3c_kernels.hpp:1504 (for (; b < B; b += gx))
    c1dw_units = 1 if fused else _ceil(7 * bsz, nch1)                        # ga3c_kernels.hpp:2149 (unit += nblk), the most of any workgroup
    tail = D1B_ROWS < bsz <= D1B_ROWS + D1B_TAIL_ROWS                        # ga3c_engine.hip:620
    trows = bsz - D1B_ROWS if tail else 0                                    # ga3c_kernels.hpp:1831
    chunks = _ceil(bsz - trows, D1B_ROWS)                                    # ga3c_kernels.hpp:1833
    last_rows = bsz - trows - D1B_ROWS * (chunks - 1)                        # ga3c_kernels.hpp:1834
    wide_w_passes = _ceil(bsz, 128)                                          # ga3c_kernels.hpp:1713 (b0 += 128; 16 waves x 8 rows a pass)
    wide_b_passes = _ceil(bsz, 1024)                                         # ga3c_kernels.hpp:1726, 1770 (b += 1024)
    # heads_bwd_role (256 threads) runs in no step: its weight columns (b0 += 32, ga3c_kernels.hpp:1265) belong to kernels kept
    # for timing; loss_sum_kernel (Network.log) is its loss role, b += 256 (ga3c_kernels.hpp:1311)
    loss_sum_passes = _ceil(bsz, 256)
    gather = "args" if bsz <= GATHER_ARGS_MAX_B else "pinned"                # ga3c_engine.hip:1147
    defer_wd = (not fused) or 2 * bsz >= fc.KSTEPS_DENSE                     # ga3c_engine.hip:731, on a fused step
    c2dx_grid = None if fused else bsz + C2DX_WD_BLOCKS                      # ga3c_engine.hip:666 (conv2_dx_wd_kernel's grid.x on a step)
    return BwdPath(fc.path(bsz), conv, nch1, nch2, c2dw_passes, c1dw_units, chunks, last_rows, tail, wide_w_passes, wide_b_passes,
                   loss_sum_passes, gather, defer_wd, c2dx_grid)


def regime(bsz):
    """bwd_path(bsz) as far as it picks code: without the trip counts and the per-row sizes (nch2 as "B" below 256)."""
    p = bwd_path(bsz)._asdict()
    p["nch2"] = "B" if p["nch2"] == bsz else p["nch2"]
    return tuple((k, v) for k, v in p.items() if k not in LOOP_FIELDS and k not in ("last_rows", "c2dx_grid"))


def changes(what, lo=161, hi=MAX_BATCH):
    """The sizes B in (lo, hi] at which what(B) differs from what(B - 1)."""
    return [b for b in range(lo + 1, hi + 1) if what(b) != what(b - 1)]


# ---------------------------------------------------------------- entries and batches
Entries = collections.namedtuple("Entries", "state y a")      # pool row of each entry, float32 return, one-hot float32 action


@functools.lru_cache(maxsize=None)
def entries(num_actions=A):
    """Entry e < 67 is pool state e with an action and a return drawn as test_gpu_parity._batch draws them (integers first,
    then U(-1, 1)), the return rounded to float32 (what the engine is handed); entries 67 .. 69 are the heavy ones."""
    rng = np.random.Generator(np.random.PCG64(ENTRY_SEED + num_actions))
    n = R + len(HEAVY)
    act = rng.integers(0, num_actions, size=n)
    y = rng.uniform(-1, 1, size=n).astype(np.float32)
    y[R:] = np.where(y[R:] >= 0, HEAVY_Y, -HEAVY_Y)
    state = np.concatenate([np.arange(R), HEAVY_STATES])
    a = np.eye(num_actions, dtype=np.float32)[act]
    for t in (state, y, a):
        t.setflags(write=False)
    return Entries(state, y, a)


@functools.lru_cache(maxsize=None)
def index(bsz):
    """forward_cases.index(bsz), the last row's entry moved on until it differs from the entries of the rows a multiple of 128
    in front of it, of row 0 and of the row before it: the rows whose data a dropped, doubled or stale last pass of a 128-,
    256-, 512- or 1024-row loop would hand it.  (Of SIZES this moves 161, 192 and 384.  At 384 rows 127 and 383 drew the same
    entry, and a conv2_dw workgroup that kept sample 127's registers for sample 383 computed the right sums.)"""
    idx = fc.index(bsz).copy()
    others = {int(idx[r]) for r in range(bsz - 1 - 128, -1, -128)} | {int(idx[0]), int(idx[-2])}
    while int(idx[-1]) in others:
        idx[-1] = (idx[-1] + 1) % R
    idx.setflags(write=False)
    return idx


def index_with(bsz, row, entry):
    """index(bsz) with `entry` at `row`."""
    idx = index(bsz).copy()
    idx[row] = entry
    idx.setflags(write=False)
    return idx


def batch(idx, ent=None):
    """-> (xk uint8, x float32, y float32, a) of the batch whose rows are the entries idx."""
    ent = entries() if ent is None else ent
    xk, x = fc.pool()
    s = ent.state[idx]
    return np.ascontiguousarray(xk[s]), np.ascontiguousarray(x[s]), np.ascontiguousarray(ent.y[idx]), np.ascontiguousarray(ent.a[idx])


# ---------------------------------------------------------------- the oracle's side
_PER_STATE = ("z", "p", "v", "s", "zs", "e", "x", "cols1", "n1", "cols2", "n2", "flat", "d1", "n1pre", "n2pre", "d1pre")


def _row(f, s):
    return {k: f[k][s:s + 1] for k in _PER_STATE}


class PoolSide:
    """The oracle on every entry at one weight set, and the tensors of any batch of those entries composed from it.

    e32 and the ReLU rule are closeness.OracleCase's, restated for a pool: e32(T) of a batch is rel_err of the float32
    composition against the float64 one evaluated with the float32 run's units; `want(idx, on)` is the float64 composition
    with the units a counterpart had on, which may differ from the oracle's only where the oracle's input to the unit is within
    bound(activation) x max|input| of zero (activation's e32 and max|input| over the pool: from 67 rows on a batch holds every
    state of it).  Copies of an entry within a batch must show the same units; only the entries whose units differ are
    evaluated again."""

    def __init__(self, params, ent, beta, fwd=None):
        """fwd: (float64, float32) forward passes of another side at the same weights (keep=True, on the pool's states)."""
        self.params = {k: np.asarray(v, np.float64) for k, v in params.items()}
        self.p32 = c.f32_params(self.params)
        self.ent, self.beta = ent, float(beta)
        self.n = ent.state.size
        if fwd is None:
            _, x = fc.pool()
            fwd = (o.forward(self.params, x.astype(np.float64), keep=True), o.forward(self.p32, x, keep=True))
        self.f, self.f32 = fwd
        self.pre = {k: self.f[k + "pre"].reshape(R, -1) for k in c.ACTS}
        self.on = {k: self.pre[k] > 0 for k in c.ACTS}
        self.on32 = {k: self.f32[k].reshape(R, -1) > 0 for k in c.ACTS}
        self.act_e32 = {k: c.rel_err(self.f32[k], self.f[k]) for k in c.ACTS}
        self.pre_scale = {k: float(np.max(np.abs(self.pre[k]))) for k in c.ACTS}
        self.own = [self._eval(e) for e in range(self.n)]
        self.g32 = [self._eval(e, f32=True) for e in range(self.n)]
        for g in self.g32:
            for k, t in g.items():
                assert t.dtype == np.float32, (k, t.dtype)          # float32 throughout, or e32 would be a lower limit only
        # the float64 entries with the float32 run's units: e32's reference
        self.ref32 = self._with_units({k: self.on32[k][ent.state] for k in c.ACTS}, np.arange(self.n))
        self._m = {}

    def _eval(self, e, on=None, f32=False):
        """One entry through o.loss_and_grads on its slice of the shared forward pass -> flat tensors + "loss" [3]."""
        s = int(self.ent.state[e])
        f, p = (self.f32, self.p32) if f32 else (self.f, self.params)
        dt = np.float32 if f32 else np.float64
        relu_on = None if on is None else {k: on[k].reshape(f[k][s:s + 1].shape) for k in c.ACTS}
        losses, g = o.loss_and_grads(p, None, self.ent.y[e:e + 1].astype(dt), self.ent.a[e:e + 1].astype(dt), dt(self.beta),
                                     relu_on=relu_on, f=_row(f, s))
        out = {k: np.asarray(g[k]).reshape(-1) for k in c.DELTAS + VARS}
        out["loss"] = np.array([losses[k] for k in LOSSES], dtype=dt)
        return out

    def _with_units(self, on, which):
        """self.own with the entries `which` evaluated for the units on[k][i] (row i belongs to which[i]) where they differ
        from the oracle's own, under closeness.OracleCase.want's condition -> (table, units that differed)."""
        table, differ = list(self.own), 0
        for i, e in enumerate(which):
            s = int(self.ent.state[e])
            d = {k: on[k][i] != self.on[k][s] for k in c.ACTS}
            n = sum(int(d[k].sum()) for k in c.ACTS)
            if n == 0:
                continue
            for k in c.ACTS:
                if d[k].any():
                    limit = c.bound(self.act_e32[k], k) * self.pre_scale[k]
                    worst = float(np.max(np.abs(self.pre[k][s][d[k]])))
                    assert worst <= limit, "%s: a unit with input %.3e is switched the other way (limit %.3e)" % (k, worst, limit)
            differ += n
            table[e] = self._eval(e, {k: on[k][i] for k in c.ACTS})
        return table, differ

    def _matrix(self, tag, table, name):
        if tag is None:
            return np.stack([t[name] for t in table])
        if (tag, name) not in self._m:
            self._m[tag, name] = np.stack([t[name] for t in table])
        return self._m[tag, name]

    def compose64(self, idx, table=None, tag=None):
        """The float64 tensors of the batch idx from a table of entries (default: the oracle's own units)."""
        if table is None:
            table, tag = self.own, "own"
        counts = np.bincount(idx, minlength=self.n).astype(np.float64)
        out = {k: self._matrix(tag, table, k)[idx] for k in c.DELTAS}
        for k in VARS + ("loss",):
            out[k] = counts @ self._matrix(tag, table, k)
        n2 = self.f["n2"].reshape(R, -1)[self.ent.state[idx]]
        out["dense1/w"] = (n2.T @ out["dd1"]).reshape(-1)
        return out

    def compose32(self, idx, order=None):
        """The float32 run's tensors of the batch idx, B float32 terms summed in float32.  order: None, the batch's own order
        (row after row); or a group count G: the kernels' slab order -- row r goes to partial sum r % G, the partial sums
        are then added pairwise as a tree."""
        out = {k: self._matrix("g32", self.g32, k)[idx] for k in c.DELTAS}
        for k in VARS + ("loss",):
            out[k] = _sum32(self._matrix("g32", self.g32, k)[idx], order)
        n2 = self.f32["n2"].reshape(R, -1)[self.ent.state[idx]]
        if order is None:
            out["dense1/w"] = (n2.T @ out["dd1"]).reshape(-1)
        else:       # the chunks of D1B_ROWS rows one after the other, each a matmul of its own
            acc = np.zeros((n2.shape[1], out["dd1"].shape[1]), np.float32)
            for c0 in range(0, idx.size, D1B_ROWS):
                acc += n2[c0:c0 + D1B_ROWS].T @ out["dd1"][c0:c0 + D1B_ROWS]
            out["dense1/w"] = acc.reshape(-1)
        for k, t in out.items():
            assert t.dtype == np.float32, (k, t.dtype)
        return out

    def e32(self, idx, order=None):
        """-> (e32 of every tensor, of the loss sums [3], of the three activations) for the batch idx."""
        ref = self.compose64(idx, self.ref32[0], "ref32")
        g32 = self.compose32(idx, order)
        e = {k: c.rel_err(g32[k], ref[k]) for k in c.TENSORS}
        # one element, a sum over the rows: a single draw of the rounding error says nothing (closeness.e32_of_row_sum)
        e["logits_v/b"] = max(e["logits_v/b"], c.e32_of_row_sum(g32["dv"], ref["dv"]))
        lrows32, lrows64 = self._matrix("g32", self.g32, "loss")[idx], self._matrix("ref32", self.ref32[0], "loss")[idx]
        loss = []
        for i in range(3):
            if ref["loss"][i] == 0.0:       # beta = 0: the entropy term is exactly zero, in float32 too
                assert g32["loss"][i] == 0.0
                loss.append(0.0)
            else:
                loss.append(max(abs(float(g32["loss"][i]) - ref["loss"][i]) / abs(ref["loss"][i]),
                                c.e32_of_row_sum(lrows32[:, i], lrows64[:, i])))
        e.update(self.act_e32)
        return e, loss

    def want(self, idx, on=None):
        """The float64 tensors of the batch idx with the ReLU units `on` (dict n1 / n2 / d1 of boolean [B, width], e.g.
        `fetched > 0`) in place of the oracle's own."""
        if on is None:
            return self.compose64(idx)
        which, first = np.unique(idx, return_index=True)
        inverse = np.searchsorted(which, idx)
        per_entry = {}
        for k in c.ACTS:
            rows = np.asarray(on[k]).reshape(idx.size, -1)
            per_entry[k] = rows[first]
            assert np.array_equal(rows, per_entry[k][inverse]), "%s: copies of a pool entry show different units" % k
        table, differ = self._with_units(per_entry, which)
        if differ == 0:
            return self.compose64(idx)
        print("%d ReLU unit(s) within rounding of zero evaluated as the counterpart had them" % differ)
        return self.compose64(idx, table)


def _sum32(rows, order):
    """Sum of the float32 rows [B, n] over B in float32: in the batch's order, or in G groups (row r to group r % G, each
    group summed in its order) and a pairwise tree over the groups."""
    assert rows.dtype == np.float32
    if order is None:
        return rows.sum(axis=0, dtype=np.float32) if rows.shape[1] > 1 else np.add.accumulate(rows[:, 0], dtype=np.float32)[-1:]
    parts = [rows[g::order].sum(axis=0, dtype=np.float32) for g in range(min(order, rows.shape[0]))]
    while len(parts) > 1:
        nxt = [parts[i] + parts[i + 1] for i in range(0, len(parts) - 1, 2)]
        if len(parts) % 2:
            nxt.append(parts[-1])
        parts = nxt
    return parts[0]


@functools.lru_cache(maxsize=None)
def side():
    """The A = 6 side at forward_cases.params("disc", 6) (logits_p/w x 40: a policy that is neither uniform nor saturated)."""
    return PoolSide(fc.params("disc", A), entries(), BETA)


def side_at(theta_flat):
    """The same entries at the weights of a float32 arena (the device's own theta' enters float64 exactly)."""
    shaped = {k: v.astype(np.float64).reshape(o.param_shapes(A)[k]) for k, v in c.split(theta_flat, A).items()}
    return PoolSide(shaped, entries(), BETA)


@functools.lru_cache(maxsize=None)
def last_row_side():
    """Only the last row has a gradient: beta = 0 and, for every entry e < 67, y = the oracle's own v of its state rounded to
    float32 (its advantage is the rounding of v, dz and dv vanish up to it); behind them one loud entry per size of
    LAST_ROW_SIZES, the entry of that batch's last row with the return entries() gave it.  -> (side, {B: idx})."""
    ent = entries()
    v = side().f["v"].astype(np.float32)
    loud = [int(index(b)[-1]) for b in LAST_ROW_SIZES]
    quiet = Entries(np.concatenate([np.arange(R), ent.state[loud]]), np.concatenate([v, ent.y[loud]]),
                    np.concatenate([ent.a[:R], ent.a[loud]]))
    idx = {}
    for i, b in enumerate(LAST_ROW_SIZES):
        idx[b] = np.concatenate([index(b)[:-1], [R + i]])
    return PoolSide(fc.params("disc", A), quiet, 0.0, (side().f, side().f32)), idx


# ---------------------------------------------------------------- bounds
# Conv gradients at 513 .. 1025 rows sum 62 k .. 410 k terms, more than the 56,448 closeness.py argues its 16 for.  A tensor that
# needs more than 16 x e32 there gets its factor here, for those sizes only, sized from the two-order ratio that
# test_backward_cases_cpu.py measures on the oracle (tests/README.md).  None needed one.
SIZE_FACTOR = {}            # (tensor name, B) -> factor


def bound(e32, name, bsz):
    return max(SIZE_FACTOR.get((name, bsz), c.FACTOR) * e32[name], c.FLOOR)


class Held:
    """What test_gpu_image_limits._check_step asks of a case: bsz, e32 per tensor, bound(name)."""

    def __init__(self, e32, bsz):
        self.e32, self.bsz = e32, bsz

    def bound(self, name):
        return bound(self.e32, name, self.bsz)


# ---------------------------------------------------------------- the wide heads
@functools.lru_cache(maxsize=None)
def wide_rows(head, num_actions, bsz):
    """-> (xk, x, a, y): the pool's states in index(bsz)'s order with targets drawn as the head's own tests draw them.  Under
    "cont" a state with an action next to atan2's branch cut or to X = Y = 0 (image_limit_cases' two rules) gives way to the
    next state that keeps away from both."""
    import continuous_oracle as co
    import image_limit_cases as ic
    idx = index(bsz).copy()
    xk, x = fc.pool()
    rng = np.random.Generator(np.random.PCG64(ENTRY_SEED + 100 * num_actions + bsz))
    if head == "cont":
        p = ic.params(head, num_actions)
        f = co.forward(p, x.astype(np.float64), keep=True)
        keep = co.safe_rows(p, x, ic.MIN_ABS_Y, f) & ((f["X"] ** 2 + f["Y"] ** 2) >= ic.FLOOR_R2).all(axis=1)
        assert keep.sum() >= ic.MIN_KEPT * R
        for i in range(bsz):
            while not keep[idx[i]]:
                idx[i] = (idx[i] + 1) % R
        a = rng.uniform(-1, 1, size=(bsz, num_actions)).astype(np.float32)
    else:
        a = np.eye(num_actions, dtype=np.float32)[rng.integers(0, num_actions, size=bsz)]
    y = rng.uniform(-1, 1, size=bsz)
    out = (np.ascontiguousarray(xk[idx]), np.ascontiguousarray(x[idx]), a, y)
    for t in out:
        t.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def wide_case(head, num_actions, bsz):
    """closeness.OracleCase / image_limit_cases.HeadCase on the materialised batch, at image_limit_cases' weights."""
    import image_limit_cases as ic
    _, x, a, y = wide_rows(head, num_actions, bsz)
    return ic.make_case(head, ic.params(head, num_actions), x, y, a)
