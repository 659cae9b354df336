"""-m gpu: the evaluation episodes of the DDPG handle (Config.DEVICE_DDPG_EVAL_ENVS, ga3c_ddpg_eval_*) against
tests/ddpg_eval_oracle.py, which tests/test_ddpg_eval_cpu.py holds to the real EnvironmentPend.Environment.  S = 3 and A = 1;
n on both sides of the 16-row tile and with a last tile of 12 rows; steps 1 (the start state's observation), 2 (the first step
that reads an observation the kernel made itself) and 200 (a whole episode, whose last step sets `done`).  Two actors: a fresh
network's, whose actions are about 1e-3, and one on which tanh saturates for part of the rows.

Exact: the action of every step (ga3c_ddpg_predict's bits on the traced observation: the same device function with the same
rows in the same tiles), the reward of every step (products and one fmod on the device's own physics and action: no
transcendental function), the thdot observation (the f32 cast), the total (the f64 sum in step order), the rewards of the stepwise
device actors started from the same states, and everything a training handle holds with and without evaluations in between.
Bounded as DESIGN.md 8l bounds one actor step, by test_gpu_ddpg_actors' PHYS_BOUND and OBS_BOUND: the physics after a step and
the cos / sin observations, whose sin and cos are the device library's and not numpy's.  `done` is not among what the kernel
stores -- an evaluation is bounded by `steps` <= 200 alone -- so it is the oracle's that says step 200 ends the episode.
Closed loop, 20 steps: TOTAL_MEASURED below."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ddpg_eval_oracle as eo
import ddpg_oracle as o
from test_gpu_ddpg import PKG, _load, _net, _same, _snapshot
from test_gpu_ddpg_actors import OBS_BOUND, PHYS_BOUND, _eq, _rel
from test_gpu_dist import _dnet
from test_gpu_prioritized_replay import _per_net
from test_gpu_td3 import _tnet

pytestmark = pytest.mark.gpu

S, A = eo.S, eo.A
SIZES = [1, 15, 16, 17, 33, 300]
STEPS = [1, 2, 200]
EINVAL, ESTATE = -1, -4
SEED = 4242
ACTOR_VARS = o.ACTOR_TRAINABLE + tuple(k for k in o.STATS if k.startswith("actor_"))
# worst |total - want| / |want| of a 20-step evaluation against the f64 oracle's rollout from the same start states, over
# test_closed_loop's inputs (every n of SIZES, both actors), measured on an MI355X.  The assertion is at 8 times
# the measured value under a cap of 1e-3: the 1e-4 that DESIGN.md 8f allows an action moves u = 2 a by 2e-4, one step's new
# speed by 3 dt 2e-4 = 3e-5 and, through the saturating test policy's gain on the observation, the later actions with it; over
# the 20 steps a 20-step total of about -20.5 moves by less than 2e-2.
TOTAL_MEASURED = 5.554e-08  # the saturating actor at n = 300; the fresh actor's worst is 8.4e-13
TOTAL_CAP = 1e-3
CLOSED_STEPS = 20


def _saturating():
    rng = np.random.Generator(np.random.PCG64(7))
    online, target = o.random_params(S, A, rng, stats=True), o.random_params(S, A, rng, stats=True)
    return online, target


def _params(net, which=0):
    """The handle's variables as the oracle takes them: f64 copies of the f32 values."""
    return {k: net.get_variable_value(k, which).astype(np.float64) for k in o.ALL_VARS}


def _handle(actor, n, **kw):
    """A handle with the `actor` ("initial": what NetworkDDPG draws; "saturating": the test weights above)."""
    net = _net(S, A, max_batch=max(16, n), capacity=max(64, 2 * n), **kw)
    if actor == "saturating":
        _load(net, *_saturating())
    return net


@pytest.mark.parametrize("actor", ["initial", "saturating"])
@pytest.mark.parametrize("steps", STEPS)
@pytest.mark.parametrize("n", SIZES)
def test_teacher_forced(n, steps, actor):
    net = _handle(actor, n)
    try:
        net.eval_create(n, seed=SEED + n, trace=True)
        start = net.eval_get("start")
        assert _eq(start, eo.start_states(SEED + n, n)) and _eq(net.eval_get("phys"), start)
        total = net.eval_run(steps)
        g = {k: net.eval_get(k) for k in ("phys", "trace_phys", "trace_obs", "trace_action", "trace_reward")}
        assert g["trace_phys"].shape == (n, 200, 2) and g["trace_obs"].shape == (n, 200, S)
        assert g["trace_action"].shape == (n, 200) and g["trace_reward"].shape == (n, 200) and total.shape == (n,)
        assert total.dtype == np.float64 and g["trace_action"].dtype == np.float32
        assert _eq(g["trace_phys"][:, 0], start)
        assert _rel(g["trace_obs"][:, 0, :2], eo.observe_many(start)[:, :2]) <= OBS_BOUND
        worst_phys = worst_obs = 0.0
        want_total = np.zeros(n, np.float64)
        for t in range(steps):
            phys, obs, action = g["trace_phys"][:, t], g["trace_obs"][:, t], g["trace_action"][:, t]
            assert _eq(action[:, None], net.predict(obs, noise=False)), t
            assert _eq(obs[:, 2], phys[:, 1].astype(np.float32)), t
            stepped, reward, _ = eo.step_many(phys, action)
            assert _eq(g["trace_reward"][:, t], reward), t
            want_total = want_total + g["trace_reward"][:, t]
            after = g["trace_phys"][:, t + 1] if t + 1 < steps else g["phys"]
            worst_phys = max(worst_phys, _rel(after, stepped))
            if t + 1 < steps:
                worst_obs = max(worst_obs, _rel(g["trace_obs"][:, t + 1, :2], eo.observe_many(after)[:, :2]))
        assert _eq(total, want_total)
        assert np.all(g["trace_reward"][:, :steps] <= -1.0) and np.all(g["trace_reward"][:, :steps] >= -1.09)
        assert np.all(np.abs(g["phys"][:, 1]) <= 8.0)
        assert worst_phys <= PHYS_BOUND, worst_phys
        assert worst_obs <= OBS_BOUND, worst_obs
        act = np.abs(g["trace_action"][:, :steps])
        if actor == "initial":
            assert act.max() < 0.05
        elif steps == 200 and n >= 15:                      # over these episodes tanh nears its ends on part of the rows, not on all
            assert (act > 0.99).any() and (act < 0.9).any()
    finally:
        net.close()


@pytest.mark.parametrize("n", [1, 17, 300])
def test_the_stepwise_device_actors_earn_the_same_rewards(n):
    steps = 40
    net, twin = _handle("saturating", n), _handle("saturating", n)
    try:
        net.eval_create(n, seed=SEED, trace=True)
        net.eval_run(steps)
        g = {k: net.eval_get(k) for k in ("start", "trace_phys", "trace_obs", "trace_action", "trace_reward")}
        twin.actors_create(n, seed=1, batch=1, updates=1)
        twin.actors_run(1, train=False, noise=False)          # step(None); then the evaluation's start, by name
        twin.actors_set("phys", g["start"])
        twin.actors_set("elapsed", np.zeros(n, np.int32))
        twin.actors_set("obs", g["trace_obs"][:, 0])
        for t in range(steps):
            assert _eq(twin.actors_get("phys"), g["trace_phys"][:, t]), t
            twin.actors_run(1, train=False, noise=False)
            assert _eq(twin.actors_get("action"), g["trace_action"][:, t:t + 1]), t
            assert _eq(twin.actors_get("reward"), g["trace_reward"][:, t]), t
    finally:
        net.close()
        twin.close()


def test_closed_loop(capsys):
    """Measured first, then asserted: the figures are printed whatever the assertion says."""
    worst, rows = 0.0, []
    for actor in ("initial", "saturating"):
        for n in SIZES:
            net = _handle(actor, n)
            try:
                net.eval_create(n, seed=SEED + n)
                got = net.eval_run(CLOSED_STEPS)
                want = eo.rollout(_params(net), net.eval_get("start"), CLOSED_STEPS)
                err = float(np.max(np.abs(got - want["total"]) / np.abs(want["total"])))
                phys = _rel(net.eval_get("phys"), want["phys"])
                rows.append((actor, n, err, phys))
                worst = max(worst, err)
            finally:
                net.close()
    with capsys.disabled():
        for actor, n, err, phys in rows:
            print("\n[ddpg eval] closed loop, %d steps, %s actor, n=%d: worst |total - want| / |want| %.3e, final physics %.3e"
                  % (CLOSED_STEPS, actor, n, err, phys), end="")
        print("\n[ddpg eval] closed loop: worst over all %.3e (TOTAL_MEASURED %r, cap %.0e)" % (worst, TOTAL_MEASURED, TOTAL_CAP))
    assert 8 * TOTAL_MEASURED <= TOTAL_CAP
    assert worst <= 8 * TOTAL_MEASURED


def _actor_state(net):
    out = {k: net.actors_get(k) for k in net.ACTOR_FIELDS}
    out.update({k: net.actors_get(k) for k in net.ACTOR_SCALARS})
    return out


@pytest.mark.parametrize("prioritized", [False, True], ids=["uniform", "prioritized"])
def test_training_is_undisturbed(prioritized):
    n, batch, capacity = 33, 16, 200
    nets = []
    try:
        for evaluating in (False, True):
            net = (_per_net(capacity, max_batch=64) if prioritized else _net(S, A, max_batch=64, capacity=capacity, RANDOM_SEED=99))
            nets.append(net)
            _load(net, *_saturating())
            net.actors_create(n, seed=31, batch=batch, updates=1, draw_seed=77)
            elapsed = 150 + np.arange(n, dtype=np.int32)      # all but two episodes end inside the run's 48 steps, on different steps
            net.actors_run(1, train=False)
            net.actors_set("elapsed", elapsed)
            if evaluating:
                net.eval_create(40, seed=5, trace=True)
            episodes, trained = [], 0
            for call in range(6):
                trained += net.actors_run(8)[1]
                episodes += net.actors_episodes()
                if evaluating:
                    totals = net.eval_run(200, target=bool(call % 2))
                    assert np.all(totals < -200.0) and np.all(totals > -218.0)
            net.result = dict(arenas=_snapshot(net), actors=_actor_state(net), step=net.get_global_step(), size=net.replay_size(),
                              ring=[net.replay_get(k) for k in range(net.replay_size()[0])], episodes=episodes, trained=trained,
                              noise=net.noise_step(), priorities=net.priorities() if prioritized else None)
        a, b = nets[0].result, nets[1].result
        assert a["trained"] == b["trained"] > 30 and a["step"] == b["step"] == a["trained"]
        assert a["size"] == b["size"] and a["size"][0] == capacity and a["size"][1] > capacity      # the ring wrapped
        assert _same(a["arenas"], b["arenas"])
        assert a["actors"].keys() == b["actors"].keys()
        for k in a["actors"]:
            assert _eq(a["actors"][k], b["actors"][k]), k
        assert all(_eq(x, y) for ra, rb in zip(a["ring"], b["ring"]) for x, y in zip(ra, rb))
        assert a["episodes"] == b["episodes"] and len(a["episodes"]) == n - 2
        assert all(_eq(x, y) for x, y in zip(a["noise"], b["noise"]))
        if prioritized:
            assert all(_eq(np.asarray(x), np.asarray(y)) for x, y in zip(a["priorities"], b["priorities"]))
    finally:
        for net in nets:
            net.close()


def test_target_reads_the_target_arena():
    n = 33
    online, target = _saturating()
    net, other = _handle("initial", n), _handle("initial", n)
    try:
        _load(net, online, target)
        _load(other, target, online)
        for h in (net, other):
            h.eval_create(n, seed=SEED)
        a0, a1 = net.eval_run(200, target=False), net.eval_run(200, target=True)
        b0, b1 = other.eval_run(200, target=False), other.eval_run(200, target=True)
        assert _eq(a1, b0) and _eq(a0, b1) and not np.array_equal(a0, a1)
    finally:
        net.close()
        other.close()


def test_repeatable_and_the_start_states_can_be_set():
    n = 33
    net = _handle("saturating", n)
    try:
        net.eval_create(n, seed=SEED, trace=True)
        first, trace = net.eval_run(200), net.eval_get("trace_reward")
        second = net.eval_run(200)
        assert _eq(first, second) and _eq(trace, net.eval_get("trace_reward"))
        assert len(set(first.tolist())) == n                 # every environment its own episode
        short = net.eval_run(7)
        want = np.zeros(n)
        for t in range(7):
            want = want + trace[:, t]
        assert _eq(short, want)                              # a shorter run is the head of the longer one
        start = net.eval_get("start")
        net.eval_set("start", start[::-1])
        assert _eq(net.eval_get("start"), np.ascontiguousarray(start[::-1]))
        moved = net.eval_run(200)
        assert _eq(net.eval_get("trace_phys")[:, 0], np.ascontiguousarray(start[::-1]))
        assert _eq(moved, np.ascontiguousarray(first[::-1]))       # a row's episode does not depend on its place in a tile
        assert _eq(net.eval_run(200), moved)
    finally:
        net.close()


def test_handle_variants_share_the_actor():
    n = 33
    online, _ = _saturating()
    plain = _handle("initial", n)
    twin = _tnet(S, A, max_batch=64, capacity=128)
    dist = _dnet(S, A, 51, max_batch=64, capacity=128)
    per = _per_net(128, max_batch=64)
    try:
        totals = []
        for net in (plain, twin, dist, per):
            for k in ACTOR_VARS:
                net.set_variable_value(k, online[k], 0)
            net.eval_create(n, seed=SEED)
            totals.append(net.eval_run(200))
            net.eval_destroy()
        assert all(_eq(t, totals[0]) for t in totals[1:])
    finally:
        for net in (plain, twin, dist, per):
            net.close()


def test_return_codes():
    import _native as nat
    lib = nat.hip_lib()
    net = _net(S, A, max_batch=16, capacity=32)
    wide = _net(7, 3, max_batch=16, capacity=32)
    out = np.zeros(4096, np.float64)
    buf = np.zeros(4096 * 400, np.float64)
    ptr, optr = buf.ctypes.data_as(C.c_void_p), nat.ptr(out, nat.f64p)
    try:
        h = net._h
        # without an evaluator: GA3C_ESTATE from every call
        assert lib.ga3c_ddpg_eval_destroy(h) == ESTATE and lib.ga3c_ddpg_eval_run(h, 200, 0, optr) == ESTATE
        assert lib.ga3c_ddpg_eval_get(h, b"start", ptr, 32) == ESTATE and lib.ga3c_ddpg_eval_set(h, b"start", ptr, 32) == ESTATE
        for n in (0, -1, 4097):
            assert lib.ga3c_ddpg_eval_create(h, n, 1, 0) == EINVAL, n
        assert lib.ga3c_ddpg_eval_create(h, 2, 1, 2) == EINVAL
        assert lib.ga3c_ddpg_eval_create(wide._h, 2, 1, 0) == EINVAL          # S = 7, A = 3
        # no device actors, more environments than max_batch or the ring's capacity: none of them is asked for
        assert lib.ga3c_ddpg_eval_create(h, 4096, 1, 0) == 0
        assert lib.ga3c_ddpg_eval_create(h, 2, 1, 0) == ESTATE
        assert lib.ga3c_ddpg_eval_run(h, 2, 0, optr) == 0 and np.all(out < -2.0) and np.all(out > -2.18)
        assert lib.ga3c_ddpg_eval_get(h, b"phys", ptr, 4096 * 16) == 0
        assert lib.ga3c_ddpg_eval_destroy(h) == 0 and lib.ga3c_ddpg_eval_destroy(h) == ESTATE
        assert lib.ga3c_ddpg_eval_create(h, 2, 1, 0) == 0
        for steps in (0, -1, 201):
            assert lib.ga3c_ddpg_eval_run(h, steps, 0, optr) == EINVAL, steps
        for target in (-1, 2):
            assert lib.ga3c_ddpg_eval_run(h, 200, target, optr) == EINVAL, target
        assert lib.ga3c_ddpg_eval_run(h, 200, 0, None) == EINVAL
        for name, size in ((b"trace_phys", 2 * 200 * 16), (b"trace_obs", 2 * 200 * 12), (b"trace_action", 2 * 200 * 4),
                           (b"trace_reward", 2 * 200 * 8)):
            assert lib.ga3c_ddpg_eval_get(h, name, ptr, size) == ESTATE, name          # created without a trace
        assert lib.ga3c_ddpg_eval_get(h, b"nothing", ptr, 8) == EINVAL
        assert lib.ga3c_ddpg_eval_get(h, b"start", ptr, 24) == EINVAL and lib.ga3c_ddpg_eval_get(h, b"start", ptr, 32) == 0
        assert lib.ga3c_ddpg_eval_set(h, b"phys", ptr, 32) == EINVAL           # read only
        assert lib.ga3c_ddpg_eval_get(h, b"elapsed_ms", ptr, 4) == ESTATE      # nothing has run
        assert lib.ga3c_ddpg_eval_run(h, 200, 1, optr) == 0
        assert lib.ga3c_ddpg_eval_get(h, b"elapsed_ms", ptr, 4) == 0 and 0.0 < net.eval_get("elapsed_ms") < 1000.0
        assert lib.ga3c_ddpg_eval_destroy(h) == 0
        assert lib.ga3c_ddpg_eval_create(h, 2, 1, 1) == 0                      # with a trace: the names exist, rows by rows
        assert lib.ga3c_ddpg_eval_get(h, b"trace_reward", ptr, 2 * 200 * 8) == 0
        assert lib.ga3c_ddpg_eval_get(h, b"trace_reward", ptr, 2 * 20 * 8) == EINVAL
        assert lib.ga3c_ddpg_eval_set(h, b"trace_reward", ptr, 2 * 200 * 8) == EINVAL
    finally:
        net.close()                                   # ga3c_ddpg_destroy with a live evaluator
        wide.close()


@pytest.mark.timeout(120)
def test_train_script_writes_the_evaluations(tmp_path):
    env = dict(os.environ, PYTHONUNBUFFERED="1")
    run = subprocess.run(["timeout", "-k", "10", "90", "sh", os.path.join(PKG, "_train.sh"), "GAME=Pendulum-v0", "USE_DDPG=True",
                          "TRAINING_MIN_BATCH_SIZE=64", "DEVICE_AGENTS=64", "DEVICE_DDPG=True", "DEVICE_DDPG_EVAL_ENVS=16",
                          "DEVICE_DDPG_EVAL_EVERY=200", "MAX_SECONDS=5"],
                         cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=110)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert "died" not in run.stdout + run.stderr
    rows = np.loadtxt(os.path.join(str(tmp_path), "logs", "network", "eval.csv"), delimiter=",", ndmin=2)
    assert rows.shape[1] == 7 and len(rows) >= 2 and rows[0, 0] == 0
    assert np.all(np.diff(rows[:, 0] // 200) >= 1)
    assert np.all(rows[:, 1] == 16) and np.all(rows[:, 2] == 200)
    assert np.all(rows[:, 4] <= rows[:, 3]) and np.all(rows[:, 3] <= rows[:, 5])
    assert np.all(rows[:, 5] <= -200.0) and np.all(rows[:, 4] >= -218.0)
    assert np.allclose(rows[:, 6], (rows[:, 3] + 200) / 0.005, rtol=0, atol=1e-9)
    # the other files keep their formats
    assert all(re.match(r"^\d{4}-\d\d-\d\d \d\d:\d\d:\d\d, -?\d+, \d+$", ln) for ln in open(os.path.join(str(tmp_path), "results.txt")))
