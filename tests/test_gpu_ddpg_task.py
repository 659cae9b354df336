"""-m gpu: the task of the DDPG device actors and evaluation episodes (Config.DEVICE_DDPG_ACTION_BOUND, _TIME_LIMIT,
_RESET_OBSERVATION, _REWARD_SCALE, _REWARD_OFFSET, ga3c_ddpg_task_*; ddpg_actors_step_kernel,
ddpg_actors_nstep_kernel, ddpg_eval_kernel with the task in their arguments, 8w) against tests/ddpg_task_oracle.py, which tests/test_ddpg_task_cpu.py holds
to ddpg_actors_oracle at the fork's task and to EnvironmentPend.Pendulum at gym's.  S = 3 and A = 1; N on both sides of the 16-row
tile of the predict kernel, in one and in two workgroups of the step kernels.

Exact: a handle with the fork's values as its task against one without a task (every arena, the ring, the discounts, every actor
field, the step, the episode records, the noise, the evaluation's totals); the action the ring keeps; reward, done, elapsed,
draws, reset physics and episode records; the ring rows around an episode's end, their discounts, and the arenas after train
steps against a twin handle fed the fetched rows.  Bounded as DESIGN.md 8l bounds one actor step, by test_gpu_ddpg_actors'
PHYS_BOUND and OBS_BOUND: the physics after a step and the cos / sin observations."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ddpg_actors_oracle as do
import ddpg_task_oracle as to
import device_pendulum_oracle as po
import nstep_oracle as ns
from test_gpu_ddpg import PKG, _load, _net, _same, _snapshot
from test_gpu_ddpg_actors import DRAW_SEED, OBS_BOUND, PHYS_BOUND, _eq, _rel, _ring_rows, _train_sizes, _weights
from test_gpu_ddpg_eval import _saturating
from test_gpu_device_pendulum import _cases
from test_gpu_prioritized_replay import _per_net

pytestmark = pytest.mark.gpu

S, A = do.S, do.A
SIZES = [1, 15, 16, 17, 33, 300]
EINVAL, ESTATE = -1, -4
GAMMA = 0.99
NOISES = (0.0, 0.8, -0.8, 3.2, -3.2)          # inside, beyond either end, more than a turn beyond either
REWARDS = [(0.005, -1.0), (1.0, 0.0), (0.1, 0.5)]
CLIP = to.FORK._replace(bound='clip')
TRUNCATE = to.FORK._replace(time_limit='truncate')


def _tasked(task, n, capacity=None, nstep=None, prioritized=False, weights=7, max_batch=None, **kw):
    """A handle with `task` attached (None: no task), n-step returns first when asked for; no actors yet."""
    max_batch = max_batch or max(16, n)
    capacity = capacity or 2 * n + 3
    net = _per_net(capacity, max_batch=max_batch, **kw) if prioritized else _net(S, A, max_batch=max_batch, capacity=capacity, **kw)
    try:
        _load(net, *_weights(weights))
        if nstep:
            net.nstep_create(nstep)
        if task is not None:
            net.task_create(*task)
            assert net.task == tuple(task) == net.task_info()
    except Exception:
        net.close()
        raise
    return net


def _ending(n, first=1):
    """elapsed for n environments of which min(5, n) end on five different steps: `first`, first + 1, ..."""
    elapsed = np.zeros(n, np.int32)
    for k, i in enumerate(range(0, n, max(1, n // 5))[:5]):
        elapsed[i] = po.TIME_LIMIT - first - k
    return elapsed


def _everything(net, trained):
    """What an actors_run can have changed, by name."""
    out = dict(_snapshot(net))
    out["ring"] = _ring_rows(net, range(net.replay_capacity))
    out["replay_size"] = np.array(net.replay_size())
    out["step"] = np.array([net.get_global_step()])
    for name in list(net.ACTOR_FIELDS) + list(net.ACTOR_SCALARS):
        if name != "slots" or trained:
            out["actors/" + name] = np.asarray(net.actors_get(name))
    if net.nstep > 1:
        out["disc"] = net.nstep_discounts()
    return out


# ---- 1. the fork's values as a task change nothing

@pytest.mark.parametrize("nstep", [1, 3])
@pytest.mark.parametrize("n", SIZES)
def test_a_fork_valued_task_changes_nothing(n, nstep):
    B = 16
    nets = [_tasked(task, n, nstep=nstep if nstep > 1 else None, weights=31) for task in (None, to.FORK)]
    try:
        episodes, trained = [], []
        for net in nets:
            net.actors_create(n, seed=77 + n, updates=1, batch=B, draw_seed=DRAW_SEED)
            net.eval_create(min(n, 17), seed=5, trace=False)
            assert net.actors_run(1, train=True) == (n, 0, 0, 0)
            net.actors_set("elapsed", _ending(n, first=3))
            stats = net.actors_run(39, train=True)             # the handle's own noise process, one seed for both
            trained.append(stats[1])
            episodes.append(net.actors_episodes())
        plain, tasked = (_everything(net, t) for net, t in zip(nets, trained))
        assert trained[0] == trained[1] and (trained[0] > 0) == (2 * n + 3 > B)
        assert set(plain) == set(tasked)
        for k in plain:
            assert _eq(plain[k], tasked[k]), k
        assert episodes[0] == episodes[1] and len(episodes[0]) == min(5, n)
        assert all(_eq(x, y) for x, y in zip(nets[0].noise_step(), nets[1].noise_step()))
        totals = [net.eval_run(200) for net in nets]
        assert _eq(totals[0], totals[1]) and np.all(totals[0] < -200.0)
    finally:
        for net in nets:
            net.close()


# ---- 2. one forced step under 'clip', and the reward's scale and offset

@pytest.mark.parametrize("n", SIZES)
def test_forced_steps_under_clip(n, capsys):
    seed = 2024 + n
    rng = np.random.Generator(np.random.PCG64(n))
    total = max(24, n)
    phys_all, elapsed_all, _ = _cases(rng, total)
    worst_phys = worst_obs = 0.0
    below = above = within = turns = 0
    for scale, offset in REWARDS:
        task = CLIP._replace(reward_scale=scale, reward_offset=offset)
        net = _tasked(task, n, weights=n)
        try:
            for g_i, nz in enumerate(NOISES):
                idx = np.arange(g_i * n, g_i * n + n) % total
                phys, elapsed = phys_all[idx].copy(), elapsed_all[idx].copy()
                draws = 2 * rng.integers(2, 1 << 39, size=n).astype(np.uint64)
                obs = rng.uniform(-1.5, 1.5, size=(n, S)).astype(np.float32)
                net.actors_create(n, seed=seed, batch=1, updates=1)
                base = net.replay_size()[1]
                assert net.actors_run(1, train=False, noise=[nz]) == (n, 0, 0, 0)          # step(None): no transition
                assert net.replay_size()[1] == base and np.all(net.actors_get("action") == 0.0)
                for name, val in (("phys", phys), ("elapsed", elapsed), ("draws", draws), ("obs", obs)):
                    net.actors_set(name, val)
                want_done = elapsed + 1 >= po.TIME_LIMIT
                assert net.actors_run(1, train=False, noise=[nz]) == (n, 0, 0, int(want_done.sum()))
                g = {k: net.actors_get(k) for k in ("phys", "elapsed", "draws", "obs", "action", "reward", "done")}
                assert _eq(g["action"], net.predict(obs, noise=[nz]))                       # as predicted: not bounded
                act = g["action"][:, 0]
                below, above, within = below + int((act < -1).sum()), above + int((act > 1).sum()), within + int((np.abs(act) <= 1).sum())
                turns += int((np.abs(act) > 3).sum())
                # the oracle's step on the device's own pre-step physics and action
                stepped, reward = zip(*[to.env_step(task, phys[i], g["action"][i]) for i in range(n)])
                stepped, reward = np.array(stepped), np.array(reward, np.float64)
                assert _eq(g["reward"], reward)
                assert np.array_equal(g["done"] != 0, want_done)
                assert np.array_equal(g["elapsed"], np.where(want_done, 0, elapsed + 1))
                assert np.array_equal(g["draws"], draws + np.uint64(2) * want_done.astype(np.uint64))
                keep = ~want_done
                worst_phys = max(worst_phys, _rel(g["phys"][keep], stepped[keep]))
                assert _eq(g["obs"][keep][:, 2], g["phys"][keep][:, 1].astype(np.float32))
                want_obs = np.array([po.PendulumEnv.observe(ph) for ph in g["phys"]])
                worst_obs = max(worst_obs, _rel(g["obs"][keep][:, :2], want_obs[keep][:, :2]))
                if want_done.any():
                    gone = np.array([po.PendulumEnv.observe(ph) for ph in stepped[want_done]])
                    worst_obs = max(worst_obs, _rel(g["obs"][want_done], gone))
                # beyond the bound the torque stays at the bound: the step of the action +-1
                for i in np.flatnonzero(np.abs(act) > 1):
                    at_bound = to.env_step(task, phys[i], np.array([np.sign(act[i])], np.float32))
                    assert _eq(np.float64(at_bound[1]), reward[i])
                # the ring rows: the action as predicted, the f32 reward, done under 'terminal'
                slots = (base + np.arange(n)) % net.replay_capacity
                want_rows = np.concatenate([obs, g["action"], reward.astype(np.float32)[:, None],
                                            want_done.astype(np.float32)[:, None], g["obs"]], axis=1)
                assert _eq(_ring_rows(net, slots), want_rows)
                assert net.actors_episodes() == [(float(reward[i]), 2) for i in np.flatnonzero(want_done)]
                net.actors_destroy()
        finally:
            net.close()
    with capsys.disabled():
        print("\n[ddpg task] N=%d: worst physics error %.3e (bound %.3e), worst cos / sin observation error %.3e (bound %.3e); "
              "actions below -1: %d, above 1: %d, within: %d, beyond +-3: %d"
              % (n, worst_phys, PHYS_BOUND, worst_obs, OBS_BOUND, below, above, within, turns))
    assert below and above and within and (turns or n == 1)
    assert worst_phys <= PHYS_BOUND
    assert worst_obs <= OBS_BOUND


# ---- 3. the time limit

def _follow(net, ora, n, steps):
    """`steps` single actor steps of `net` under given noise, the oracle re-seeded from the device's physics and observation and
    stepped with the device's action each time.  Checks reward, done, elapsed, draws, the reset physics and the episode records
    -> [(step, the oracle's outputs, the device's fields, the oracle's rows, ended, the observations before the step)]."""
    seen = []
    for step in range(steps):
        nz = NOISES[step % len(NOISES)] * (0.5 + 0.01 * step)
        before_phys, before_obs = net.actors_get("phys"), net.actors_get("obs")
        stats = net.actors_run(1, train=False, noise=[nz])
        g = {k: net.actors_get(k) for k in ("phys", "obs", "action", "reward", "done", "elapsed", "draws")}
        for i, e in enumerate(ora.env):
            e.phys, e.obs = before_phys[i].copy(), before_obs[i].copy()
        rows, eps, outs = ora.step(g["action"])
        assert stats == (n, 0, 0, len(eps))
        assert _eq(g["reward"], np.array([r["reward"] for r in outs], np.float64))
        assert np.array_equal(g["done"] != 0, np.array([r["done"] for r in outs]))            # `ended`, whatever the task
        assert np.array_equal(g["elapsed"], np.array([e.elapsed for e in ora.env], np.int32))
        assert np.array_equal(g["draws"], np.array([e.rng.draws for e in ora.env], np.uint64))
        ended = np.array([r["episode"] is not None for r in outs])
        assert _eq(g["phys"][ended], np.array([e.phys for e in ora.env])[ended].reshape(-1, 2))   # the reset's draws
        assert _rel(g["phys"][~ended], np.array([e.phys for e in ora.env])[~ended]) <= PHYS_BOUND
        assert net.actors_episodes() == eps
        seen.append((step, outs, g, rows, ended, before_obs))
    return seen


@pytest.mark.parametrize("limit", ["truncate", "terminal"])
@pytest.mark.parametrize("n", SIZES)
def test_the_time_limit(n, limit):
    task = to.FORK._replace(time_limit=limit)
    seed, capacity = 300 + n, 12 * n
    net = _tasked(task, n, capacity=capacity)
    try:
        net.actors_create(n, seed=seed, batch=1, updates=1)
        ora = to.Actors(n, seed, task)
        assert net.actors_run(1, train=False, noise=[0.0]) == (n, 0, 0, 0)
        ora.step(None)
        elapsed = _ending(n)
        elapsed[elapsed == 0] = 1                                      # (step(None) counted one)
        net.actors_set("elapsed", elapsed)
        for e, el in zip(ora.env, elapsed):
            e.elapsed = int(el)
        ends = 0
        for step, outs, g, rows, ended, before_obs in _follow(net, ora, n, 8):
            slots = (step * n + np.arange(n)) % capacity
            got = _ring_rows(net, slots)
            # s2 is the observation the step made, before any reset; without reset_observation the field keeps it
            want = np.concatenate([before_obs, g["action"], g["reward"].astype(np.float32)[:, None],
                                   (ended & (limit == "terminal")).astype(np.float32)[:, None], g["obs"]], axis=1)
            assert _eq(got, want), step
            assert all(_eq(got[i, S + A + 1], rows[i][3]) for i in range(n))
            ends += int(ended.sum())
            if ended.any():
                assert step in range(5) and np.all(got[ended, S + A + 1] == (1.0 if limit == "terminal" else 0.0))
        assert ends == min(5, n)
    finally:
        net.close()


@pytest.mark.parametrize("reset", [True, False], ids=["restart", "continue"])
def test_the_noise_restarts_where_a_truncated_episode_ends(reset):
    import envnoise_oracle as eo
    n = 33
    net = _tasked(TRUNCATE, n)
    try:
        net.actors_create(n, seed=44, batch=1, updates=1, noise='per_env', noise_seed=97531, noise_reset=reset)
        net.actors_run(1, train=False)
        elapsed = _ending(n)
        net.actors_set("elapsed", elapsed)
        net.actors_set("noise_x", np.full((n, A), 0.5, np.float32))       # far from 0: a restart cannot be mistaken for a step
        restarted = 0
        for c in range(8):
            before, done = net.actors_get("noise_x"), net.actors_get("done")
            net.actors_run(1, train=False)
            x, drawn = net.actors_get("noise_x"), net.actors_get("noise_n")
            assert _eq(x, eo.step(before, drawn, done, reset)), c
            after = done != 0
            if after.any():
                restarted += int(after.sum())
                from_zero = eo.step(np.zeros((int(after.sum()), A), np.float32), drawn[after])
                assert _eq(x[after], from_zero) == reset
        assert restarted == 5
        rows = _ring_rows(net, range(net.replay_size()[0]))
        assert np.all(rows[:, S + A + 1] == 0.0)
    finally:
        net.close()


# ---- 4. reset_observation

@pytest.mark.parametrize("n", SIZES)
def test_reset_observation(n):
    seed, capacity = 500 + n, 12 * n
    fresh, stale = (_tasked(to.FORK._replace(reset_observation=flag), n, capacity=capacity) for flag in (True, False))
    try:
        for net in (fresh, stale):
            net.actors_create(n, seed=seed, batch=1, updates=1)
            net.actors_run(1, train=False, noise=[0.0])
            net.actors_set("elapsed", _ending(n))
        was_reset = np.zeros(n, bool)
        ends, worst = 0, 0.0
        for step in range(8):
            nz = [NOISES[step % len(NOISES)]]
            obs_before = {id(net): net.actors_get("obs") for net in (fresh, stale)}
            for net in (fresh, stale):
                net.actors_run(1, train=False, noise=nz)
            f, s = ({k: net.actors_get(k) for k in ("phys", "obs", "done", "reward")} for net in (fresh, stale))
            ended = f["done"] != 0
            assert np.array_equal(ended, s["done"] != 0)
            slots = (step * n + np.arange(n)) % capacity
            rf, rs = _ring_rows(fresh, slots), _ring_rows(stale, slots)
            # a row starts with the bits of the obs field before the step: the reset state's after a reset, or the stale ones
            assert _eq(rf[:, :S], obs_before[id(fresh)]) and _eq(rs[:, :S], obs_before[id(stale)])
            same = ~was_reset                                  # environments that have not been reset yet run alike in both
            assert _eq(rf[same], rs[same]) and _eq(f["reward"][same], s["reward"][same])
            # s2 of an ending row: the observation before the reset, which the handle without the option keeps in its field
            assert _eq(rf[ended & same, S + A + 2:], s["obs"][ended & same])
            assert _eq(s["obs"], rs[:, S + A + 2:])
            assert _eq(f["obs"][~ended], rf[~ended, S + A + 2:])
            if ended.any():
                ends += int(ended.sum())
                assert _eq(f["phys"][ended & same], s["phys"][ended & same])          # the same reset draws
                want = np.array([po.PendulumEnv.observe(ph) for ph in f["phys"][ended]])
                assert _eq(f["obs"][ended][:, 2], want[:, 2])
                worst = max(worst, _rel(f["obs"][ended][:, :2], want[:, :2]))
                assert not np.array_equal(f["obs"][ended], s["obs"][ended])
            was_reset |= ended
        assert ends >= min(5, n) and worst <= OBS_BOUND
    finally:
        fresh.close()
        stale.close()


# ---- 5. n-step returns across a truncated end

@pytest.mark.parametrize("n", SIZES)
def test_nstep_rows_around_a_truncated_end(n):
    nstep, seed, capacity, steps = 3, 700 + n, 14 * n, 12
    net = _tasked(TRUNCATE, n, capacity=capacity, nstep=nstep)
    try:
        net.actors_create(n, seed=seed, batch=1, updates=1)
        ora = to.NStepActors(n, seed, nstep, GAMMA, TRUNCATE)
        ring = ns.Ring(capacity, False, GAMMA)
        assert net.actors_run(1, train=False, noise=[0.0]) == (n, 0, 0, 0)
        ora.step(None)
        elapsed = _ending(n, first=2)
        elapsed[elapsed == 0] = 1
        net.actors_set("elapsed", elapsed)
        for e, el in zip(ora.env, elapsed):
            e.elapsed = int(el)
        ends = 0
        for step in range(steps):
            nz = NOISES[step % len(NOISES)] * (0.5 + 0.01 * step)
            before_phys, before_obs = net.actors_get("phys"), net.actors_get("obs")
            stats = net.actors_run(1, train=False, noise=[nz])
            g = {k: net.actors_get(k) for k in ("obs", "action", "reward", "done")}
            for i, e in enumerate(ora.env):
                e.phys, e.obs = before_phys[i].copy(), before_obs[i].copy()
            pairs, eps, outs = ora.step(g["action"], s2=g["obs"])
            assert stats == (n, 0, 0, len(eps)) and net.actors_episodes() == eps
            assert _eq(g["reward"], np.array([r["reward"] for r in outs], np.float64))
            assert np.array_equal(g["done"] != 0, np.array([r["done"] for r in outs]))
            assert len(pairs) == (n if step >= nstep - 1 else 0)
            ring.add([p[0] for p in pairs], [p[1] for p in pairs])
            ends += len(eps)
            assert net.replay_size() == (ring.size, ring.total)
        assert ends == min(5, n) and ring.total == (steps - nstep + 1) * n <= capacity
        rows, disc = _ring_rows(net, range(ring.size)), net.nstep_discounts()
        assert _eq(rows, ring.rows[:ring.size])                      # R, done = 0, s2 of the last transition summed
        assert _eq(disc, ring.disc)                                  # (f32) gamma^m
        assert np.all(rows[:, S + A + 1] == 0.0)
        short = disc[:ring.size] != np.float32(ns.gamma64(GAMMA) * ns.gamma64(GAMMA) * ns.gamma64(GAMMA))
        assert int(short.sum()) == 2 * min(5, n)                     # the two transitions before each end: m = 2 and m = 1
    finally:
        net.close()


# ---- 6. train steps after task steps

@pytest.mark.parametrize("prioritized", [False, True], ids=["uniform", "prioritized"])
def test_train_steps_after_task_steps_are_the_twins(prioritized):
    """test_gpu_ddpg_actors' method: the twin has no task and no actors; it is fed the rows the task wrote."""
    n, capacity, steps, B, noise = 17, 400, 8, 16, [0.3]
    net = _tasked(to.GYM, n, capacity=capacity, prioritized=prioritized, weights=31, max_batch=64)
    twin = _tasked(None, n, capacity=capacity, prioritized=prioritized, weights=31, max_batch=64)
    try:
        net.replay_beta = twin.replay_beta = 0.4
        start = _snapshot(net)
        net.actors_create(n, seed=5, updates=1, batch=B, draw_seed=DRAW_SEED)
        assert net.actors_run(1, train=True, noise=noise) == (n, 0, 0, 0)
        net.actors_set("elapsed", _ending(n, first=2))
        sizes = _train_sizes(n, B, steps, 1)
        assert net.actors_run(steps, train=True, noise=noise) == (n * steps, len(sizes), len(sizes) * B, 5)
        assert net.replay_size() == (n * steps, n * steps)
        rows = _ring_rows(net, range(n * steps))
        assert np.all(rows[:, S + A + 1] == 0.0) and np.all(rows[:, S + A] <= 0.0) and np.any(rows[:, S + A] < -1.09)
        sample, q_twin, last_slots = 0, None, None
        for k in range(steps):
            f = rows[k * n:(k + 1) * n]
            size, _ = twin.replay_add(f[:, :S], f[:, S:S + A], f[:, S + A], f[:, S + A + 1], f[:, S + A + 2:])
            if size > B:
                assert size == sizes[sample]
                if prioritized:
                    q_twin = twin.train_prioritized(B, noise=noise)
                    last_slots = twin.last_slots
                else:
                    last_slots = do.uniform_slots(DRAW_SEED, sample, size, B)
                    q_twin = twin.train_replay(last_slots, noise=noise)
                sample += 1
        assert sample == len(sizes) >= 6
        assert np.array_equal(net.actors_get("slots"), last_slots)
        assert net.logging == q_twin
        assert _same(_snapshot(net), _snapshot(twin)) and not _same(start, _snapshot(net))
        assert net.get_global_step() == twin.get_global_step() == len(sizes)
        if prioritized:
            (pa, top), (tpa, ttop) = net.priorities(), twin.priorities()
            assert top == ttop and _eq(pa, tpa)
    finally:
        net.close()
        twin.close()


# ---- 7. evaluation episodes

@pytest.mark.parametrize("n", SIZES)
def test_evaluation_under_gyms_reward_teacher_forced(n):
    task = to.FORK._replace(reward_scale=1.0, reward_offset=0.0)
    net = _net(S, A, max_batch=max(16, n), capacity=max(64, 2 * n))
    try:
        _load(net, *_saturating())
        net.task_create(*task)
        net.eval_create(n, seed=4242 + n, trace=True)
        total = net.eval_run(200)
        g = {k: net.eval_get(k) for k in ("phys", "trace_phys", "trace_obs", "trace_action", "trace_reward")}
        want_total = np.zeros(n, np.float64)
        worst = 0.0
        for t in range(200):
            stepped, reward, _ = to.step_many(task, g["trace_phys"][:, t], g["trace_action"][:, t])
            assert _eq(g["trace_reward"][:, t], reward), t          # the oracle's bits on the device's own physics and action
            want_total = want_total + g["trace_reward"][:, t]
            worst = max(worst, _rel(g["trace_phys"][:, t + 1] if t < 199 else g["phys"], stepped))
        assert _eq(total, want_total)                               # the f64 sum in step order
        assert worst <= PHYS_BOUND
        assert np.all(g["trace_reward"] <= 0.0) and np.any(g["trace_reward"] < -1.09)      # gym's units
    finally:
        net.close()


# ---- 8. return codes

def test_return_codes_and_lifetimes():
    import _native as nat
    lib = nat.hip_lib()
    net = _net(S, A, max_batch=16, capacity=40)
    b, t, r = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    sc, off = C.c_double(), C.c_double()

    def create(bound=0, limit=0, reset=0, scale=0.005, offset=-1.0):
        return lib.ga3c_ddpg_task_create(net._h, bound, limit, reset, scale, offset)

    def info():
        return lib.ga3c_ddpg_task_info(net._h, C.byref(b), C.byref(t), C.byref(r), C.byref(sc), C.byref(off))
    try:
        h = net._h
        assert lib.ga3c_ddpg_task_destroy(h) == ESTATE and info() == ESTATE          # without a task
        assert lib.ga3c_ddpg_task_create(None, 0, 0, 0, 1.0, 0.0) == EINVAL
        for bad in (dict(bound=2), dict(bound=-1), dict(limit=2), dict(limit=-1), dict(reset=2), dict(reset=-1),
                    dict(scale=0.0), dict(scale=-1.0), dict(scale=float("inf")), dict(scale=float("nan")),
                    dict(offset=float("nan")), dict(offset=float("inf")), dict(offset=float("-inf"))):
            assert create(**bad) == EINVAL, bad
        assert info() == ESTATE                                                      # ... and none of them attached one
        assert create() == 0                                                         # the fork's values are accepted
        assert create() == ESTATE and create(1, 1, 1, 1.0, 0.0) == ESTATE            # a second create
        assert info() == 0 and (b.value, t.value, r.value, sc.value, off.value) == (0, 0, 0, 0.005, -1.0)
        assert lib.ga3c_ddpg_task_info(h, None, None, None, None, None) == 0         # each pointer may be null
        assert lib.ga3c_ddpg_task_destroy(h) == 0 and lib.ga3c_ddpg_task_destroy(h) == ESTATE
        assert create(1, 1, 1, 0.1, 0.5) == 0
        assert info() == 0 and (b.value, t.value, r.value, sc.value, off.value) == (1, 1, 1, 0.1, 0.5)
        # live actors or a live evaluator: the task can neither go nor come
        net.actors_create(8, seed=1, batch=1, updates=1)
        assert lib.ga3c_ddpg_task_destroy(h) == ESTATE and info() == 0
        net.actors_destroy()
        net.eval_create(4)
        assert lib.ga3c_ddpg_task_destroy(h) == ESTATE
        net.eval_destroy()
        assert lib.ga3c_ddpg_task_destroy(h) == 0
        net.actors_create(8, seed=1, batch=1, updates=1)
        assert create() == ESTATE
        net.actors_destroy()
        net.eval_create(4)
        assert create() == ESTATE
        net.eval_destroy()
        assert create(1, 1, 1, 1.0, 0.0) == 0
        net.actors_create(8, seed=1, batch=1, updates=1)
        net.eval_create(4)
        assert net.actors_run(3, train=False) == (24, 0, 0, 0) and np.all(net.eval_run(5) <= 0.0)
    finally:
        net.close()                                   # ga3c_ddpg_destroy with a live task, live actors and a live evaluator


# ---- 9. the product line

LINE = ["GAME=Pendulum-v0", "USE_DDPG=True", "TRAINING_MIN_BATCH_SIZE=64", "DEVICE_AGENTS=64", "DEVICE_DDPG=True", "MAX_SECONDS=2"]
GYM_LINE = ["DEVICE_DDPG_ACTION_BOUND=clip", "DEVICE_DDPG_TIME_LIMIT=truncate", "DEVICE_DDPG_RESET_OBSERVATION=True",
            "DEVICE_DDPG_REWARD_SCALE=1", "DEVICE_DDPG_REWARD_OFFSET=0"]
DEFAULT_LINE = ["DEVICE_DDPG_ACTION_BOUND=wrap", "DEVICE_DDPG_TIME_LIMIT=terminal", "DEVICE_DDPG_RESET_OBSERVATION=",
                "DEVICE_DDPG_REWARD_SCALE=0.005", "DEVICE_DDPG_REWARD_OFFSET=-1.0"]


def _train(tmp_path, name, extra):
    cwd = tmp_path / name
    cwd.mkdir()
    run = subprocess.run(["timeout", "-k", "10", "90", "sh", os.path.join(PKG, "_train.sh")] + LINE + extra, cwd=str(cwd),
                         env=dict(os.environ, PYTHONUNBUFFERED="1"), capture_output=True, text=True, timeout=110)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "died" not in run.stdout + run.stderr
    lines = open(str(cwd / "results.txt")).read().strip().splitlines()
    records = [(ln.split(",")[1].strip(), int(ln.split(",")[2])) for ln in lines]
    assert len(records) >= 64 and all(length in (200, 201) for _, length in records)
    return cwd, records


@pytest.mark.timeout(120)
def test_train_script_runs_gyms_task(tmp_path):
    cwd, records = _train(tmp_path, "gym", GYM_LINE + ["DEVICE_DDPG_EVAL_ENVS=16", "DEVICE_DDPG_EVAL_EVERY=200"])
    assert all(-16.3 * 200 <= float(r) <= 0.0 for r, _ in records) and any(float(r) < -218.0 for r, _ in records)
    rows = np.loadtxt(str(cwd / "logs" / "network" / "eval.csv"), delimiter=",", ndmin=2)
    assert rows.shape[1] == 7 and len(rows) >= 1 and rows[0, 0] == 0
    assert np.all(rows[:, 1] == 16) and np.all(rows[:, 2] == 200)
    assert np.all(rows[:, 5] <= 0.0) and np.all(rows[:, 4] >= -16.3 * 200)
    assert np.array_equal(rows[:, 6], rows[:, 3])     # mean_gym_return = (mean - 200 * 0) / 1: the return is in gym's units


@pytest.mark.timeout(120)
def test_the_line_without_the_keys_is_the_line_with_the_defaults(tmp_path):
    (_, plain), (_, spelt) = _train(tmp_path, "plain", []), _train(tmp_path, "defaults", DEFAULT_LINE)
    k = min(len(plain), len(spelt))
    assert plain[:k] == spelt[:k]
    assert all(-1.09 * 200 <= float(r) <= -199 for r, _ in plain)
