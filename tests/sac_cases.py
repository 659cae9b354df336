"""The cases of tests/test_gpu_sac.py and the choice of their rows (not collected: no test_ prefix), shared with
tests/test_sac_cpu.py, which runs the choice for every case without a GPU and asserts that each finds its rows.

The rule is test_gpu_td3._select's: 4 B candidate rows are drawn, and the first B are kept that satisfy, in the f64 oracle
(tests/sac_oracle.py), under the draws of their place in the batch,
  * every relu unit of every evaluation of the step more than 1e-4 from zero (a unit closer than that could land on the other
    side of zero in f32): sac_oracle.relu_margin, and on a policy step sac_oracle.policy_margin after the critics' step;
  * on a policy step |q1 - q2| > 1e-4 x max(1, |q|): the smaller critic is selected per row, and a closer pair could select the
    other one in f32.
A row that fails gives its place to the next candidate not yet tried, so the others keep their places and their draws.

The policy step's evaluations come after the critics' step, which depends on the whole batch: replacing one row moves every
unit of both critics for every row.  A soft step has eight evaluations (the twin's has six, and after its critics' step only
critic 1's second layer), and at the critics' usual rate (10 x 3e-4, RMSProp) that movement is of the band's own size, so the
choice does not settle inside 4 B candidates: rows that qualified stop qualifying as others are replaced.  The cases keep the
rule and the cap and make the movement small against the band instead:
  * the single-step cases (every row, saturation, selection, priorities, n-step), which compare rows and gradients and no
    weight after a step, run at ROWS_LR = 3e-6;
  * the three-step cases, which hold weights and slots to 1e-5 after steps and so need steps that are larger than that, run at
    LR = 3e-4 with Config.critic_lr = 1 (STEPS_CRITIC_LR): the critics' elements then move by 3e-4 x their gradient.
tests/test_sac_cpu.py asserts that every case finds its rows within the cap."""
import numpy as np

import sac_oracle as so

LR = 3e-4
ROWS_LR = 3e-6
STEPS_CRITIC_LR = 1.0
SEED = 12345                      # Config.RANDOM_SEED; NetworkDDPG hands RANDOM_SEED + 3 to soft_create
SOFT_SEED = SEED + 3
SHAPES = [(3, 1), (7, 3), (3, 16)]
SIZES = [1, 15, 16, 17, 33]
EVERY_ROW = [(S, A, B) for S, A in SHAPES for B in SIZES] + [(7, 3, 132)]
STEP_WAYS = {"rmsprop": dict(), "adam": dict(RMSPROP=False), "clip": dict(USE_GRAD_CLIP=True)}
STEP_CASES = [(way, delay) for way in STEP_WAYS for delay in (1, 2)]
STEPS_B, STEPS_SHAPE, STEPS = 33, (7, 3), 3


def candidates(S, A, n, rng):
    """test_gpu_ddpg._candidates' rows."""
    return (rng.uniform(-1.5, 1.5, (n, S)).astype(np.float32), rng.uniform(-1, 1, (n, A)).astype(np.float32),
            rng.uniform(-1, 0, n).astype(np.float32), (rng.uniform(size=n) < 0.25).astype(np.float32),
            rng.uniform(-1.5, 1.5, (n, S)).astype(np.float32))


def f64(batch):
    return tuple(np.asarray(t, np.float64) for t in batch)


def copy_state(st):
    return dict(st, online={k: v.copy() for k, v in st["online"].items()}, target=dict(st["target"]),
                slot_a={k: v.copy() for k, v in st["slot_a"].items()}, slot_b={k: v.copy() for k, v in st["slot_b"].items()})


def oracle_kw(cfg):
    """Config settings -> sac_oracle.train_step's keyword arguments (test_gpu_ddpg._cfg_kw's without the loss form)."""
    return dict(critic_rmsprop=cfg.get("RMSPROP", True), momentum=cfg.get("RMSPROP_MOMENTUM", 0.0),
                clip=40.0 if cfg.get("USE_GRAD_CLIP") else None, future=cfg.get("DDPG_FUTURE_REWARD_CALC", True))


def select(st, cand, B, policy_delay=1, per_w=None, lr=LR, **kw):
    """-> (the B chosen rows, how many candidates were tried)."""
    n, A = cand[1].shape
    assert n == 4 * B
    t = st["step"] + 1
    eps2, eps = so.step_draws(SOFT_SEED, t, B, A)
    place, tried = np.full(B, -1), 0
    for _ in range(60):
        need = np.flatnonzero(place < 0)
        assert tried + need.size <= n, "only %d of %d candidate rows qualify" % (B - need.size, n)
        place[need] = np.arange(tried, tried + need.size)
        tried += need.size
        rows = f64(tuple(c[place] for c in cand))
        bad = so.relu_margin(st["online"], st["target"], rows[0], rows[1], rows[4], eps2) <= 1e-4
        if not bad.any() and t % policy_delay == 0:
            trial = copy_state(st)
            so.train_step(trial, *rows, lr, policy_delay=policy_delay, eps2=eps2, eps=eps, per_w=per_w, stop_after=3, **kw)
            margin, gap = so.policy_margin(trial["online"], rows[0], eps)
            bad = (margin <= 1e-4) | (gap <= 1e-4)
        if not bad.any():
            return tuple(c[place] for c in cand), tried
        place[bad] = -1
    raise AssertionError("the choice of rows did not settle")


def every_row_case(S, A, B):
    """Test 1's weights and rows -> (online, target, batch, tried)."""
    rng = np.random.Generator(np.random.PCG64(300 + B + S + A))
    online, target = so.random_params(S, A, rng, stats=True), so.random_params(S, A, rng, stats=True)
    batch, tried = select(so.new_state(online, target), candidates(S, A, 4 * B, rng), B, 1, lr=ROWS_LR)
    return online, target, batch, tried


def steps_kw(way):
    return dict(oracle_kw(STEP_WAYS[way]), critic_lr=STEPS_CRITIC_LR)


def steps_case(way, delay):
    """Test 3's weights, oracle state and random stream -> (online, target, st, rng); each step's rows are
    select(st, candidates(S, A, 4 B, rng), B, delay, **steps_kw(way)) on the state as it then stands."""
    S, A = STEPS_SHAPE
    rng = np.random.Generator(np.random.PCG64(502))
    online, target = so.random_params(S, A, rng), so.random_params(S, A, rng)
    st = so.new_state(online, target, critic_rmsprop=STEP_WAYS[way].get("RMSPROP", True))
    return online, target, st, rng


SATURATION_LS = (2.0, 30.0, -20.0, -60.0, 0.0)      # the raw ls of action i: at ls_max, beyond it, at ls_min, beyond it, inside


def saturation_case(S=7, A=5, B=17):
    """Test 4's weights and rows: the head's bias puts the means at +-9 (and one at 0.5) and, the head's ls columns being zero, the
    raw ls at exactly SATURATION_LS."""
    rng = np.random.Generator(np.random.PCG64(901))
    online, target = so.random_params(S, A, rng, stats=True), so.random_params(S, A, rng, stats=True)
    w = online["actor_output/W"] * 0.01
    w[:, A:] = 0.0
    online["actor_output/W"] = w.astype(np.float32).astype(np.float64)
    online["actor_output/b"] = np.array([9.0, -9.0, 9.0, -9.0, 0.5] + list(SATURATION_LS))
    batch, tried = select(so.new_state(online, target), candidates(S, A, 4 * B, rng), B, 1, lr=ROWS_LR)
    return online, target, batch, tried


def selection_case(shift, S=7, A=3, B=17):
    """Test 5's weights and rows: critic2_output/b shifted by `shift` in the online net."""
    rng = np.random.Generator(np.random.PCG64(902))
    online, target = so.random_params(S, A, rng, stats=True), so.random_params(S, A, rng, stats=True)
    online["critic2_output/b"] = online["critic2_output/b"] + shift
    batch, tried = select(so.new_state(online, target), candidates(S, A, 4 * B, rng), B, 1, lr=ROWS_LR)
    return online, target, batch, tried
