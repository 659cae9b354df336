"""The cases of tests/test_image_limits_cpu.py and tests/test_gpu_image_limits.py (not collected: no test_ prefix): the image
net at the action counts ga3c_net_create admits (num_actions 1 .. 64, 1 .. 32 under CONTINUOUS_INPUT).  Both files build their
cases here, so the conditions the CPU file asserts are the conditions of the rows the GPU file runs.

    HEADS                     "disc" (softmax head), "cont" (CONTINUOUS_INPUT, 2A columns), "dual" (DUAL_RMSPROP)
    ACTIONS[head]             both sides of launch_heads' seams (npc <= 8 | <= 24 | <= 64), the limit, an odd stride next to it
    sizes(head, A)            1 and 17 for every A; 97, 121 and 129 as well at the limit shapes
    rows(head, A, B)          the rows of the existing _batch recipes (the continuous ones with a floor under X^2 + Y^2)
    case(head, A, B)          closeness.OracleCase, or HeadCase: the same statement for the continuous head and the two costs
    forward_case(...)         p, v, z of the float64 oracle and e32 of each

No case or condition here touches a kernel; a condition is the float64 oracle's statement about the rows."""
import contextlib
import functools

import numpy as np

import closeness as c
import continuous_oracle as co
import dual_oracle as d
import ga3c_oracle as o
import test_gpu_backward_relative as tbr
import test_gpu_dual_rmsprop as tdr
import test_gpu_params_and_saturation as tps

BETA = 0.01
HEADS = ("disc", "cont", "dual")
ACTIONS = {"disc": (1, 8, 9, 24, 25, 63, 64), "cont": (4, 5, 12, 13, 31, 32), "dual": (9, 25, 64)}
LIMIT = {"disc": (63, 64), "cont": (32,), "dual": (64,)}
MAX_BATCH = 136                       # 129 is the largest batch; the handles of every file are sized a little above theirs
CONT_SEED = 4321                      # continuous_oracle.init_params(A, seed=4321), as tests/test_gpu_continuous.py
MIN_ABS_Y, FLOOR_R2, MIN_KEPT = 1e-3, 1e-5, 0.60
NEAR = ((13, 17), (32, 17))           # (A, B) of the continuous cases that keep the rows below FLOOR_R2
NEAR_FROM, NEAR_MIN_ROWS = 129, 3     # ... taken from the candidates of this size's draw; at least so many are in the batch
SOFTMAX = {"default": {}, "log_softmax": dict(USE_LOG_SOFTMAX=True), "min_policy": dict(MIN_POLICY=0.01)}
SOFTMAX_A, SOFTMAX_B = (25, 64), 17
SATURATED = {25: 9000, 64: 9032}      # A -> seed of test_gpu_params_and_saturation._saturated (SCALE = 200, 32 rows)
SAT_SHARE = (0.1, 0.9)                # the clamped share; that file's 0.7 does not hold at 64 columns (0.71 there)

# A tensor whose kernel needs more than closeness.FACTOR has its factor here, with the reason from its summation length.
# v, dv = v - y_r and logits_v/b on a batch of ONE row, and only there: each is then ONE element, v = b + sum_k d1_k Wv_k over
# K = 256 products (dv the same sum minus y_r, logits_v/b the "sum" of that one dv).  A single draw of the float32 oracle can
# come out at one rounding of the result while another order of the same K terms has the typical error of the sum, about
# sqrt(K) roundings: sqrt(256) = 16 on top of the 16 that every tensor has (tests/test_gpu_vector_limits.ONE_ROW_FACTOR, K = 64
# there).  z at A = 1, B = 1 is the same kind of element (z_0 = b + sum_k d1_k Wp_k0, K = 256) and is held the same way.
ONE_ROW_FACTOR = c.FACTOR * 16.0
ONE_ROW = ("v", "z", "dv", "logits_v/b", "v:logits_v/b")


def sizes(head, num_actions):
    """The heads run one wave per row, so the batch reaches them through other paths only (the 128-row stride of the role
    kernels' batch loops, the sites of the fused update, the conv and dense1 paths in front); none of those knows A but
    through the number of roles, which is largest at the limit.  The large sizes therefore go to the limit shapes, where an
    oracle case costs a quarter of a second; every other A runs at 1 and 17 rows."""
    return (1, 17, 97, 121, 129) if num_actions in LIMIT[head] else (1, 17)


CASES = [(h, A, B) for h in HEADS for A in ACTIONS[h] for B in sizes(h, A)]


@contextlib.contextmanager
def config(**kw):
    """Config with the given settings for the length of the block."""
    import ga3c_amd  # noqa: F401
    from Config import Config
    saved = {k: getattr(Config, k) for k in kw}
    for k, v in kw.items():
        setattr(Config, k, v)
    try:
        yield Config
    finally:
        for k, v in saved.items():
            setattr(Config, k, v)


def order(head):
    return co.PARAM_ORDER if head == "cont" else o.PARAM_ORDER


def shapes(head, num_actions):
    return co.param_shapes(num_actions) if head == "cont" else o.param_shapes(num_actions)


@functools.lru_cache(maxsize=None)
def params(head, num_actions):
    """The weights of the existing files; the tests copy before they step them."""
    return co.init_params(num_actions, seed=CONT_SEED) if head == "cont" else o.init_params(num_actions)


def flat(head, p):
    return np.concatenate([np.asarray(p[k]).reshape(-1) for k in order(head)])


def split(head, arena, num_actions):
    """flat arena -> dict of flat tensors in the head's PARAM_ORDER."""
    out, off = {}, 0
    for name in order(head):
        size = int(np.prod(shapes(head, num_actions)[name]))
        out[name] = np.asarray(arena[off:off + size])
        off += size
    assert off == np.asarray(arena).size
    return out


def unflat(head, arena, num_actions):
    """flat float32 arena -> float64 params (exact)."""
    return {k: v.astype(np.float64).reshape(shapes(head, num_actions)[k]) for k, v in split(head, arena, num_actions).items()}


# ---------------------------------------------------------------- rows
@functools.lru_cache(maxsize=None)
def _cont_draw(num_actions, bsz, seed):
    """The draws of test_gpu_continuous._batch (same generator, same order) -> (xk, x, kept by safe_rows, kept by the floor, a,
    y): safe_rows' rule |Y| >= 1e-3 where X < 0 (and radius >= 1e-3) is continuous_oracle's own; the floor asks
    X^2 + Y^2 >= FLOOR_R2 of every action of a row, because dz carries 1 / (X^2 + Y^2) and below it float32 loses X itself."""
    p = params("cont", num_actions)
    rng = np.random.Generator(np.random.PCG64(seed))
    xk = rng.integers(0, 256, size=(2 * bsz + 16, 84, 84, 4), dtype=np.uint8)
    x = xk.astype(np.float32) / np.float32(128.0) - np.float32(1.0)
    f = co.forward(p, x.astype(np.float64), keep=True)
    safe = co.safe_rows(p, x, MIN_ABS_Y, f)
    above = ((f["X"] ** 2 + f["Y"] ** 2) >= FLOOR_R2).all(axis=1)
    a = rng.uniform(-1, 1, size=(bsz, num_actions)).astype(np.float32)
    y = rng.uniform(-1, 1, size=bsz)
    return xk, x, safe, above, a, y


def cont_kept(num_actions, bsz):
    """-> (candidate rows both rules keep, candidate rows)."""
    _, _, safe, above, _, _ = _cont_draw(num_actions, bsz, 200 + bsz)
    return int((safe & above).sum()), int(safe.size)


@functools.lru_cache(maxsize=None)
def rows(head, num_actions, bsz, near=False):
    """-> (xk uint8, x float32, a, y) of one case; `near` (continuous only): the rows below the floor are kept."""
    if head == "disc":
        xk, x, a, y = tbr._batch(bsz, num_actions, 300 + bsz)
    elif head == "dual":
        xk, x, a, y = tdr._batch(bsz, num_actions, 1000 + bsz)
    elif near:
        # the 2 B + 16 candidates of B = 17 hold 0 and 1 rows that safe_rows keeps and the floor does not (radius in
        # [1e-3, 3.2e-3)); the 274 candidates of the B = 129 draw hold 6 and 3: those first, then rows above the floor
        xk, x, safe, above, a, y = _cont_draw(num_actions, NEAR_FROM, 200 + NEAR_FROM)
        pick = np.concatenate([np.flatnonzero(safe & ~above), np.flatnonzero(safe & above)])[:bsz]
        xk, x, a, y = xk[pick], x[pick], a[:bsz].copy(), y[:bsz].copy()
    else:
        xk, x, safe, above, a, y = _cont_draw(num_actions, bsz, 200 + bsz)
        keep = safe & above
        xk, x = xk[keep][:bsz], x[keep][:bsz]
        assert x.shape[0] == bsz
    for t in (xk, x, a, y):
        t.setflags(write=False)
    return xk, x, a, y


def rows_below_floor(num_actions, bsz):
    """How many rows of rows("cont", A, B, near=True) have an action with X^2 + Y^2 < FLOOR_R2, and the smallest radius."""
    _, x, _, _ = rows("cont", num_actions, bsz, True)
    f = co.forward(params("cont", num_actions), x.astype(np.float64), keep=True)
    r2 = f["X"] ** 2 + f["Y"] ** 2
    return int((r2 < FLOOR_R2).any(axis=1).sum()), float(np.sqrt(r2.min()))


# ---------------------------------------------------------------- the oracle's side of a case
class HeadCase:
    """closeness.OracleCase for the continuous head ("cont": continuous_oracle, 5 deltas + 12 variables) and for the two costs of
    DUAL_RMSPROP ("dual": dual_oracle; dz, dv, then each cost's dd1 / dn2 / dn1 and ten variables as "p:<name>" and "v:<name>",
    exactly zero where a cost cannot reach a tensor).  Same fields and the same rules: the float64 tensors, e32 of every tensor
    from a run that is float32 throughout, and the float64 tensors re-evaluated for a counterpart's ReLU units, which may differ
    only where the oracle's input to them is within the activation's bound of zero."""

    def __init__(self, head, p, x, y, a, beta):
        assert head in ("cont", "dual")
        self.head = head
        self.params = {k: np.asarray(v, np.float64) for k, v in p.items()}
        self.x = np.asarray(x, np.float32).reshape(-1, o.H, o.W, o.C)
        self.y = np.asarray(y, np.float32)
        self.a = np.asarray(a, np.float32)
        self.beta = float(beta)
        self.bsz = self.x.shape[0]
        fwd = co.forward if head == "cont" else o.forward
        f = fwd(self.params, self.x.astype(np.float64), keep=True)
        self.pre = {k: f[k + "pre"].reshape(self.bsz, -1) for k in c.ACTS}
        self.on = {k: self.pre[k] > 0 for k in c.ACTS}
        self.losses, self.g = self._grads(None, f)
        self.tensors = tuple(self.g)
        p32 = c.f32_params(self.params)
        f32 = fwd(p32, self.x, keep=True)
        _, g32 = self._run(p32, self.x, self.y, self.a, None, f32)          # (each forward pass is run once)
        pk = "o" if head == "cont" else "p"
        self.fwd = {"p": np.asarray(f[pk]), "v": np.asarray(f["v"]), "z": np.asarray(f["z"])}
        self.fwd32 = {"p": np.asarray(f32[pk]), "v": np.asarray(f32["v"]), "z": np.asarray(f32["z"])}
        for k in self.tensors:
            assert np.asarray(g32[k]).dtype == np.float32, (k, np.asarray(g32[k]).dtype)
        self.e32 = {k: c.rel_err(f32[k], f[k]) for k in c.ACTS}
        ref = self.want({k: f32[k].reshape(self.bsz, -1) > 0 for k in c.ACTS})
        for k in self.tensors:
            if np.any(ref[k]):
                self.e32[k] = c.rel_err(g32[k], ref[k])
                if k.endswith("logits_v/b"):      # one element, a sum over the rows: closeness.e32_of_row_sum
                    self.e32[k] = max(self.e32[k], c.e32_of_row_sum(g32["dv"], ref["dv"]))
            else:
                assert not np.any(g32[k]), k
                self.e32[k] = 0.0
        self.g32 = {k: np.asarray(g32[k]) for k in self.tensors}

    def _run(self, p, x, y, a, relu_on, f=None):
        if self.head == "cont":
            losses, g = co.loss_and_grads(p, x, y, a, self.beta, relu_on=relu_on, f=f)
            return losses, {k: np.asarray(g[k]) for k in c.DELTAS + co.PARAM_ORDER}
        losses, gp, gv = d.dual_grads(p, x, y, a, self.beta, relu_on=relu_on, f=f)
        out = {"dz": np.asarray(gp["dz"]), "dv": np.asarray(gv["dv"])}
        for tag, g in (("p:", gp), ("v:", gv)):
            out.update({tag + k: np.asarray(g[k]) for k in ("dd1", "dn2", "dn1") + o.PARAM_ORDER})
        return losses, out

    def _grads(self, relu_on, f=None):
        return self._run(self.params, self.x.astype(np.float64), self.y.astype(np.float64), self.a.astype(np.float64), relu_on, f)

    def bound(self, name):
        return c.bound(self.e32[name], name)

    def want(self, on=None):
        if on is None:
            return self.g
        on = {k: np.asarray(on[k]).reshape(self.bsz, -1) for k in c.ACTS}
        differ = 0
        for k in c.ACTS:
            dk = on[k] != self.on[k]
            differ += int(dk.sum())
            if dk.any():
                limit = self.bound(k) * float(np.max(np.abs(self.pre[k])))
                worst = float(np.max(np.abs(self.pre[k][dk])))
                assert worst <= limit, "%s: a unit with input %.3e is switched the other way (limit %.3e)" % (k, worst, limit)
        if differ == 0:
            return self.g
        print("%d ReLU unit(s) within rounding of zero evaluated as the counterpart had them" % differ)
        return self._grads(on)[1]


def make_case(head, p, x, y, a, beta=BETA):
    if head == "disc":
        case = c.OracleCase(p, x, y, a, beta)
        case.tensors = c.TENSORS
        return case
    return HeadCase(head, p, x, y, a, beta)


@functools.lru_cache(maxsize=None)
def case(head, num_actions, bsz, near=False):
    """The oracle's side of rows(head, A, B) at params(head, A): computed once, shared, left unchanged."""
    _, x, a, y = rows(head, num_actions, bsz, near)
    return make_case(head, params(head, num_actions), x, y, a)


def bound(cs, name, size=None):
    """closeness' bound of one tensor of a case; ONE_ROW_FACTOR for the one-element tensors of a one-row batch."""
    if cs.bsz == 1 and name in ONE_ROW and (size is None or size == 1):
        return max(ONE_ROW_FACTOR * cs.e32[name], c.FLOOR)
    return cs.bound(name)


def zero_tensors(head, num_actions):
    """The tensors that are exactly zero in the oracle, in float32 as in float64, and so on the GPU."""
    if head == "dual":
        return tuple("p:" + k for k in d.HEAD_V) + tuple("v:" + k for k in d.HEAD_P)
    if head == "disc" and num_actions == 1:        # one action: the softmax is 1 and has no gradient
        return ("dz", "logits_p/w", "logits_p/b")
    return ()


class ForwardCase:
    """p (the action vector under "cont"), v and z of the float64 oracle on the rows, and e32 of each from the float32 run."""

    def __init__(self, head, p, x, min_policy=0.0, use_log_softmax=False, case=None):
        x = np.asarray(x, np.float32)
        self.bsz = x.shape[0]
        if case is not None:      # the two forward passes the case has run already
            f, f32 = case.fwd, case.fwd32
        elif head == "cont":
            f, f32 = co.forward(p, x.astype(np.float64)), co.forward(c.f32_params(p), x)
            f, f32 = dict(f, p=f["o"]), dict(f32, p=f32["o"])
        else:
            f = o.forward(p, x.astype(np.float64), min_policy, use_log_softmax)
            f32 = o.forward(c.f32_params(p), x, np.float32(min_policy), use_log_softmax)
        self.want = {k: np.asarray(f[k]) for k in ("p", "v", "z")}
        for k in self.want:
            assert np.asarray(f32[k]).dtype == np.float32, k
        self.e32 = {k: c.rel_err(f32[k], f[k]) for k in self.want}

    def bound(self, name):
        return c.bound(self.e32[name], name)


@functools.lru_cache(maxsize=None)
def forward_case(head, num_actions, bsz, softmax="default", near=False):
    kw = {"default": {}, "log_softmax": dict(use_log_softmax=True), "min_policy": dict(min_policy=0.01)}[softmax]
    _, x, _, _ = rows(head, num_actions, bsz, near)
    return ForwardCase(head, params(head, num_actions), x, case=case(head, num_actions, bsz, near) if softmax == "default" else None, **kw)


# ---------------------------------------------------------------- the optimizer, as the engine states it
DECAY, EPS = 0.99, 0.1                # Config.RMSPROP_DECAY / RMSPROP_EPSILON (the GPU file asserts them)
# Two production steps from ms = 0, mom = 0.  The first at the rate the project trains with, so that the second starts from
# weights next to the seeded ones (one step of LR_PROBE from ms = 0 moves every entry with |g| > 3 by 0.4 and the continuous
# head's sigmoids overflow: tests/test_image_limits_cpu.py); the second at tests/test_gpu_step_probe.py's LR_PROBE, at which
# every entry that needs a sign has a step above its weight's ulp.
LR_SMALL, LR_PROBE = 3e-4, 0.05
MOMENTUM = 0.5


def want_step(g, ms, lr):
    """test_gpu_step_probe._want_step: the RMSProp step for gradient g from slot ms with the engine's float32 constants
    -> (ms', step)."""
    omr = np.float64(np.float32(1.0) - np.float32(DECAY))
    ms_new = ms + (g * g - ms) * omr
    return ms_new, g * np.float64(np.float32(lr)) / np.sqrt(np.float64(np.float32(EPS)) + ms_new)


def step_slope(ms, ms_new, lr):
    """d step / d g of want_step, elementwise: lr (eps + (1 - omr) ms) / (eps + ms')^1.5 -- how an error of g reaches the step."""
    omr = np.float64(np.float32(1.0) - np.float32(DECAY))
    eps = np.float64(np.float32(EPS))
    t = eps + ms_new
    return np.float64(np.float32(lr)) * (eps + (1.0 - omr) * ms) / (t * np.sqrt(t))


def clip_norm(head, g):
    """A GRAD_CLIP_NORM that bites on every variable (tf.clip_by_average_norm clips where ||g|| / n > clip): half the
    smallest ||g|| / n over the variables with a gradient, as tests/test_gpu_continuous.py picks it; float32, as the engine
    is handed it."""
    norms = [np.sqrt(np.sum(np.asarray(g[k], np.float64) ** 2)) / np.size(g[k]) for k in order(head) if np.any(g[k])]
    return float(np.float32(0.5 * min(norms)))


def variant_sizes(head, num_actions):
    """The batch sizes of the momentum and the clipped variant of a shape."""
    return (17, 129) if num_actions in LIMIT[head] else (17,)


@functools.lru_cache(maxsize=None)
def clip_norm_of(head, num_actions):
    """One GRAD_CLIP_NORM per (head, A), so that one handle serves the shape: the smallest clip_norm over its sizes."""
    return min(clip_norm(head, case(head, num_actions, bsz).g) for bsz in variant_sizes(head, num_actions))


def oracle_theta1(head, num_actions, bsz, variant, lr=LR_SMALL):
    """The float32 weights after the oracle's own first step of a variant (what the CPU file looks at; the GPU file takes the
    device's own theta' instead)."""
    cs = case(head, num_actions, bsz)
    p = params(head, num_actions)
    clip = clip_norm_of(head, num_actions) if variant == "clip" else None
    out = {}
    for k in order(head):
        if head == "dual":
            step = np.zeros(p[k].size)
            for tag, heads in (("v:", d.HEAD_P), ("p:", d.HEAD_V)):
                if k not in heads:
                    step = step + want_step(np.asarray(cs.g[tag + k], np.float64).reshape(-1), 0.0, lr)[1]
        else:
            g = np.asarray(cs.g[k], np.float64).reshape(-1)
            if clip is not None:
                g = o.clip_by_average_norm(g, clip)
            step = want_step(g, 0.0, lr)[1]
        out[k] = (p[k].reshape(-1) - step).astype(np.float32).astype(np.float64).reshape(p[k].shape)
    return out


# ---------------------------------------------------------------- the saturated policy
@functools.lru_cache(maxsize=None)
def saturated(num_actions):
    """test_gpu_params_and_saturation._saturated at the wide heads -> (params, xk, x, a, y)."""
    return tps._saturated(num_actions, SATURATED[num_actions])


def check_saturated(num_actions, eps=1e-6):
    """That file's conditions on the case, from the float64 oracle, with the clamped share held to SAT_SHARE -> figures."""
    p, _, x, a, _ = saturated(num_actions)
    p64 = o.forward(p, x.astype(np.float64))["p"]
    sel = (p64 * a).sum(axis=1)
    share = float((p64 < eps).mean())
    nearest = float(np.min(np.abs(p64 / eps - 1.0)))
    assert p64.min() < 1e-9 and p64.max() > 0.9999 and SAT_SHARE[0] < share < SAT_SHARE[1], (num_actions, share)
    assert (sel < eps).sum() >= 4 and (sel >= eps).sum() >= 4, (num_actions, int((sel < eps).sum()))
    assert nearest > 0.01, (num_actions, nearest)
    return dict(share=share, clamped_rows=int((sel < eps).sum()), open_rows=int((sel >= eps).sum()), nearest=nearest,
                min_p=float(p64.min()), max_p=float(p64.max()))
