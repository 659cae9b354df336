"""-m gpu: per-environment exploration noise of the DDPG device actors (Config.DEVICE_DDPG_NOISE = 'per_env',
ga3c_ddpg_envnoise_*) against tests/envnoise_oracle.py, which tests/test_envnoise_cpu.py holds to what its draws
must be.  S = 3 and A = 1; N on both sides of the 16-row tile of the predict kernel and in more than one workgroup, and at N = 17
max_batch = 17, so that the last tile's live row is the last element of every buffer the epilogue touches.

Exact: the state x' (the oracle's step fed the device's own previous state and its own draw: products and sums in f64, one cast),
the action (f32 sum of ga3c_ddpg_predict's bits without noise on the device's own observation and x'), the ring row's action, the
count, everything a train step leaves (against a twin handle), and what the other noise modes leave alone.
Within one f32 spacing of the wanted value: the draw n.  Its f64 log and cos are the device library's and not numpy's; they may
differ in the last place of the f64 product, whose cast to f32 may then fall on the other side of a rounding boundary.  Nothing
else may differ."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ddpg_actors_oracle as do
import device_pendulum_oracle as po
import envnoise_oracle as eo
from test_gpu_ddpg import PKG, _load, _net, _same, _snapshot
from test_gpu_ddpg_actors import DRAW_SEED, OBS_BOUND, PHYS_BOUND, _eq, _rel, _ring_rows, _train_sizes, _weights
from test_gpu_prioritized_replay import _per_net

pytestmark = pytest.mark.gpu

S, A = do.S, do.A
SIZES = [1, 15, 16, 17, 33, 300]
EINVAL, ESTATE = -1, -4
NOISE_SEED = 97531
FIELDS = ("noise_x", "noise_n", "noise_count")
ZERO = [0.0] * A


def _handle(n, reset=False, seed=NOISE_SEED, capacity=None, prioritized=False, batch=1, weights=7, **kw):
    """A handle whose n device actors have per-environment noise; max_batch = n at 17."""
    max_batch = kw.pop("max_batch", n if n == 17 else max(16, n))
    capacity = capacity or 2 * n + 3
    net = _per_net(capacity, max_batch=max_batch, **kw) if prioritized else _net(S, A, max_batch=max_batch, capacity=capacity, **kw)
    try:
        _load(net, *_weights(weights))
        net.actors_create(n, seed=11 + n, batch=batch, updates=1, draw_seed=DRAW_SEED, noise='per_env', noise_seed=seed,
                          noise_reset=reset)
    except Exception:
        net.close()
        raise
    return net


def _noise(net):
    return {k: net.actors_get(k) for k in FIELDS}


def _same_noise(a, b):
    return _eq(a["noise_x"], b["noise_x"]) and _eq(a["noise_n"], b["noise_n"]) and a["noise_count"] == b["noise_count"]


def _within_one_spacing(got, want):
    return bool(np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)))


@pytest.mark.parametrize("n", SIZES)
def test_six_steps_draw_step_and_act_as_the_oracle(n):
    net = _handle(n)
    try:
        start = _noise(net)
        assert start["noise_x"].shape == (n, A) and start["noise_x"].dtype == np.float32 and start["noise_n"].shape == (n, A)
        assert np.all(start["noise_x"] == 0) and np.all(start["noise_n"] == 0) and start["noise_count"] == 0
        assert net.actors_run(1, train=False) == (n, 0, 0, 0)            # step(None): no prediction, nothing counted or drawn
        assert _same_noise(_noise(net), start) and np.all(net.actors_get("action") == 0.0)
        exact = 0
        for c in range(6):
            before, obs, base = net.actors_get("noise_x"), net.actors_get("obs"), net.replay_size()[1]
            net.actors_run(1, train=False)
            g = _noise(net)
            want_n = eo.draws(NOISE_SEED, n, c, A)
            assert _within_one_spacing(g["noise_n"], want_n), c
            exact += int(np.sum(g["noise_n"] == want_n))
            assert _eq(g["noise_x"], eo.step(before, g["noise_n"])), c
            action = net.actors_get("action")
            assert _eq(action, net.predict(obs, noise=ZERO) + g["noise_x"]), c
            assert g["noise_count"] == c + 1
            slots = (base + np.arange(n)) % net.replay_capacity
            assert net.replay_size()[1] == base + n and _eq(_ring_rows(net, slots)[:, S:S + A], action), c
        assert exact >= 6 * n * A - max(1, (6 * n * A) // 16)           # the rounding boundary is met rarely, if at all
    finally:
        net.close()


def test_the_ring_row_of_an_n_step_handle_carries_the_action_of_its_first_transition():
    n, steps = 17, 3
    net = _handle(n, capacity=400, DDPG_NSTEP=steps)
    try:
        net.actors_run(1, train=False)
        actions = []
        for c in range(7):
            base, obs = net.replay_size()[1], net.actors_get("obs")
            net.actors_run(1, train=False)
            x = net.actors_get("noise_x")
            actions.append(net.actors_get("action"))
            assert _eq(actions[-1], net.predict(obs, noise=ZERO) + x) and net.actors_get("noise_count") == c + 1
            if c < steps - 1:
                assert net.replay_size()[1] == base == 0
            else:
                assert net.replay_size()[1] == base + n
                assert _eq(_ring_rows(net, base + np.arange(n))[:, S:S + A], actions[c - steps + 1]), c
    finally:
        net.close()


def test_the_shared_process_is_untouched_and_the_environments_explore_apart():
    n, k = 300, 5
    per, idle, shared, mirror = _handle(n), _net(S, A), _net(S, A, max_batch=n, capacity=2 * n + 3), _net(S, A)
    try:
        _load(shared, *_weights(7))
        shared.actors_create(n, seed=11 + n, batch=1, updates=1)
        for net in (per, shared):
            net.actors_run(1, train=False)
        for step in range(k):
            obs = {net: net.actors_get("obs") for net in (per, shared)}
            for net in (per, shared):
                net.actors_run(1, train=False)
            # what the feature is for: every environment is pushed its own way
            x = per.actors_get("noise_x")
            moved = per.actors_get("action").astype(np.float64) - per.predict(obs[per], noise=ZERO).astype(np.float64)
            assert len(np.unique(x)) == n and len(np.unique(moved)) == n, step
            # ... where the shared process pushes all of them one way: by its state v, up to the rounding of the f32 sum
            v, _ = mirror.noise_step()
            assert _eq(shared.actors_get("action"), shared.predict(obs[shared], noise=v)), step
            moved = shared.actors_get("action").astype(np.float64) - shared.predict(obs[shared], noise=ZERO).astype(np.float64)
            assert np.max(np.abs(moved - np.float64(v[0]))) <= 2.0 ** -23, step
        a, b, c = per.noise_step(), idle.noise_step(), shared.noise_step()
        assert _eq(a[0], b[0]) and _eq(a[1], b[1])                        # k per-environment steps took no step of it
        assert not np.array_equal(a[1], c[1])                             # k shared steps did
    finally:
        for net in (per, idle, shared, mirror):
            net.close()


def test_set_states_reach_both_wrap_branches_and_the_environment_step_follows_the_oracle():
    n = 33
    net = _handle(n)
    try:
        net.actors_run(1, train=False)
        values = np.array([0.8, -0.8, 3.2, -3.2, 0.0], np.float32)
        x0 = values[np.arange(n) % 5][:, None]
        net.actors_set("noise_x", x0)
        assert _eq(net.actors_get("noise_x"), x0)
        obs = np.random.Generator(np.random.PCG64(n)).uniform(-1.5, 1.5, size=(n, S)).astype(np.float32)
        net.actors_set("obs", obs)                                        # a tanh output that varies under every value
        phys = net.actors_get("phys")
        net.actors_run(1, train=False)
        g = {k: net.actors_get(k) for k in ("phys", "obs", "action", "reward", "done", "noise_x", "noise_n")}
        assert _eq(g["noise_x"], eo.step(x0, g["noise_n"]))
        assert _eq(g["action"], net.predict(obs, noise=ZERO) + g["noise_x"])
        act = g["action"][:, 0]
        # both branches of the environment's wrap, more than a turn beyond an end, and no wrap at all
        assert (act > 1).any() and (act < -1).any() and (np.abs(act) > 3).any() and (np.abs(act) <= 1).any()
        stepped, reward = zip(*[do.env_step(phys[i], g["action"][i]) for i in range(n)])
        stepped, reward = np.array(stepped), np.array(reward, np.float64)
        assert _eq(g["reward"], reward) and np.all(reward <= -1.0) and np.all(reward >= -1.09)
        assert not g["done"].any()
        assert _rel(g["phys"], stepped) <= PHYS_BOUND
        assert _eq(g["obs"][:, 2], g["phys"][:, 1].astype(np.float32))
        want_obs = np.array([po.PendulumEnv.observe(ph) for ph in g["phys"]])
        assert _rel(g["obs"][:, :2], want_obs[:, :2]) <= OBS_BOUND
    finally:
        net.close()


@pytest.mark.parametrize("reset", [True, False], ids=["reset", "continue"])
def test_reset_on_done(reset):
    n = 33
    net = _handle(n, reset=reset)
    try:
        net.actors_run(1, train=False)
        elapsed = np.zeros(n, np.int32)
        for i in range(n):
            if i % 3 != 2:
                elapsed[i] = po.TIME_LIMIT - 2 - i % 5                    # these episodes end inside the run, on different steps
        net.actors_set("elapsed", elapsed)
        net.actors_set("noise_x", np.full((n, A), 0.5, np.float32))       # far from 0: a restart cannot be mistaken for a step
        ended_on, restarted = set(), 0
        for c in range(9):
            before, done = net.actors_get("noise_x"), net.actors_get("done")
            net.actors_run(1, train=False)
            g = _noise(net)
            assert _eq(g["noise_x"], eo.step(before, g["noise_n"], done, reset)), c
            after_done = done != 0
            if after_done.any():
                ended_on.add(c)
                restarted += int(after_done.sum())
                from_zero = eo.step(np.zeros((int(after_done.sum()), A), np.float32), g["noise_n"][after_done])
                carried_on = eo.step(before[after_done], g["noise_n"][after_done])
                assert not np.array_equal(from_zero, carried_on)
                assert _eq(g["noise_x"][after_done], from_zero if reset else carried_on), c
            assert _eq(g["noise_x"][~after_done], eo.step(before[~after_done], g["noise_n"][~after_done])), c
        assert restarted == int(np.sum(elapsed > 0)) and len(ended_on) >= 4
    finally:
        net.close()


@pytest.mark.parametrize("prioritized", [False, True], ids=["uniform", "prioritized"])
def test_train_steps_are_the_twins(prioritized):
    """test_gpu_ddpg_actors' method under the handle's own noise: the predictions take the environments' processes, every train
    step's step 4 one step of the shared process, which the twin -- it predicts nothing -- takes in its train steps alike."""
    n, capacity, steps, B = 17, 400, 8, 16
    net = _handle(n, capacity=capacity, prioritized=prioritized, batch=B, weights=31, max_batch=64)
    twin = _per_net(capacity, max_batch=64) if prioritized else _net(S, A, max_batch=64, capacity=capacity)
    mirror = _net(S, A)
    try:
        net.replay_beta = twin.replay_beta = 0.4
        _load(twin, *_weights(31))
        start = _snapshot(net)
        adds = steps
        sizes = _train_sizes(n, B, adds, 1)
        assert net.actors_run(1 + steps, train=True) == (n * (1 + steps), len(sizes), len(sizes) * B, 0)
        assert net.actors_get("noise_count") == steps and net.replay_size() == (n * adds, n * adds)
        rows = _ring_rows(net, range(n * adds))
        assert len(np.unique(rows[:, S:S + A])) == n * adds               # the rows' actions: every environment its own, every step
        sample, q_twin, last_slots = 0, None, None
        for k in range(adds):
            f = rows[k * n:(k + 1) * n]
            size, _ = twin.replay_add(f[:, :S], f[:, S:S + A], f[:, S + A], f[:, S + A + 1], f[:, S + A + 2:])
            if size > B:
                assert size == sizes[sample]
                if prioritized:
                    q_twin = twin.train_prioritized(B)
                    last_slots = twin.last_slots
                else:
                    last_slots = do.uniform_slots(DRAW_SEED, sample, size, B)
                    q_twin = twin.train_replay(last_slots)
                sample += 1
        assert sample == len(sizes) >= 6
        assert np.array_equal(net.actors_get("slots"), last_slots)
        assert net.logging == q_twin
        assert _same(_snapshot(net), _snapshot(twin)) and not _same(start, _snapshot(net))
        assert net.get_global_step() == twin.get_global_step() == len(sizes)
        # step 4 is 8f's: the last train step added the shared process's state to all of its rows
        for _ in range(len(sizes)):
            v, _ = mirror.noise_step()
        assert _eq(net.fetch("a_noisy", B * A), net.fetch("a_out", B * A) + v[0])
        assert all(_eq(x, y) for x, y in zip(net.noise_step(), twin.noise_step()))
        if prioritized:
            (pa, top), (tpa, ttop) = net.priorities(), twin.priorities()
            assert top == ttop and _eq(pa, tpa)
    finally:
        for h in (net, twin, mirror):
            h.close()


def test_given_and_none_leave_the_noise_alone():
    n = 33
    net = _handle(n)
    try:
        net.actors_run(3, train=False)
        held = _noise(net)
        assert held["noise_count"] == 2 and np.all(held["noise_x"] != 0)
        obs = net.actors_get("obs")
        net.actors_run(1, train=False, noise=[0.3])
        assert _eq(net.actors_get("action"), net.predict(obs, noise=[0.3])) and _same_noise(_noise(net), held)
        obs = net.actors_get("obs")
        net.actors_run(1, train=False, noise=False)
        assert _eq(net.actors_get("action"), net.predict(obs, noise=False)) and _same_noise(_noise(net), held)
        net.actors_run(2, train=False, noise=[-0.1])
        assert _same_noise(_noise(net), held)
        before = held["noise_x"]
        net.actors_run(1, train=False)                                    # ... and the own mode goes on from where it was
        g = _noise(net)
        assert g["noise_count"] == 3 and _eq(g["noise_x"], eo.step(before, g["noise_n"]))
        assert _within_one_spacing(g["noise_n"], eo.draws(NOISE_SEED, n, 2, A))
    finally:
        net.close()


def test_determinism_and_replay():
    n = 33
    ends = []
    for seed in (NOISE_SEED, NOISE_SEED, NOISE_SEED + 1):
        net = _handle(n, seed=seed)
        try:
            net.actors_run(41, train=False)                               # step(None) and 40 predictions
            ends.append((_noise(net), net.actors_get("action")))
            if seed != NOISE_SEED:
                continue
            x0, c0 = net.actors_get("noise_x"), net.actors_get("noise_count")
            net.actors_run(1, train=False)
            x1, n1 = net.actors_get("noise_x"), net.actors_get("noise_n")
            net.actors_run(2, train=False)
            net.actors_set("noise_x", x0)
            net.actors_set("noise_count", c0)
            net.actors_run(1, train=False)
            assert _eq(net.actors_get("noise_x"), x1) and _eq(net.actors_get("noise_n"), n1)
            assert net.actors_get("noise_count") == c0 + 1 == 41
        finally:
            net.close()                                                   # destroy with live noise
    assert _same_noise(ends[0][0], ends[1][0]) and _eq(ends[0][1], ends[1][1]) and ends[0][0]["noise_count"] == 40
    assert not np.array_equal(ends[0][0]["noise_x"], ends[2][0]["noise_x"])
    assert not np.array_equal(ends[0][0]["noise_n"], ends[2][0]["noise_n"])


def test_return_codes_and_lifetimes():
    import ga3c_amd  # noqa: F401
    import _native as nat
    lib = nat.hip_lib()
    n = 20
    net = _net(S, A, max_batch=32, capacity=64)
    quiet = _net(S, A, max_batch=32, capacity=64, add_OUnoise=False)
    buf = np.zeros(n * A, np.float32)
    word = np.zeros(1, np.int64)
    ptr, wptr = buf.ctypes.data_as(C.c_void_p), word.ctypes.data_as(C.c_void_p)

    def nothing_named(h, code):
        for name, p, size in ((b"noise_x", ptr, 4 * n * A), (b"noise_n", ptr, 4 * n * A), (b"noise_count", wptr, 8)):
            assert lib.ga3c_ddpg_actors_get(h, name, p, size) == code, name
            assert lib.ga3c_ddpg_actors_set(h, name, p, size) == code, name
    try:
        h = net._h
        # without device actors: the buffers are sized by their number
        assert lib.ga3c_ddpg_envnoise_create(h, 1, 0) == ESTATE and lib.ga3c_ddpg_envnoise_destroy(h) == ESTATE
        nothing_named(h, ESTATE)
        assert lib.ga3c_ddpg_actors_create(h, n, 1, 1) == 0
        # actors without per-environment noise
        assert lib.ga3c_ddpg_envnoise_destroy(h) == ESTATE
        nothing_named(h, ESTATE)
        for flag in (2, -1, 256):
            assert lib.ga3c_ddpg_envnoise_create(h, 1, flag) == EINVAL, flag
        nothing_named(h, ESTATE)
        assert lib.ga3c_ddpg_envnoise_create(h, 1, 1) == 0
        assert lib.ga3c_ddpg_envnoise_create(h, 1, 1) == ESTATE
        # by name
        assert lib.ga3c_ddpg_actors_get(h, b"noise_x", ptr, 4 * n * A) == 0 and np.all(buf == 0)
        assert lib.ga3c_ddpg_actors_get(h, b"noise_x", ptr, 4 * n * A - 4) == EINVAL
        assert lib.ga3c_ddpg_actors_get(h, b"noise_n", ptr, 4 * n * A + 4) == EINVAL
        assert lib.ga3c_ddpg_actors_get(h, b"noise_count", wptr, 4) == EINVAL
        assert lib.ga3c_ddpg_actors_set(h, b"noise_n", ptr, 4 * n * A) == EINVAL          # read only
        for bad in (np.nan, np.inf, -np.inf):
            buf[:] = 0.25
            buf[-1] = bad
            assert lib.ga3c_ddpg_actors_set(h, b"noise_x", ptr, 4 * n * A) == EINVAL, bad
        buf[:] = 0
        assert lib.ga3c_ddpg_actors_get(h, b"noise_x", ptr, 4 * n * A) == 0 and np.all(buf == 0)      # ... and nothing was set
        buf[:] = 0.25
        assert lib.ga3c_ddpg_actors_set(h, b"noise_x", ptr, 4 * n * A) == 0
        word[0] = -1
        assert lib.ga3c_ddpg_actors_set(h, b"noise_count", wptr, 8) == EINVAL
        word[0] = 7
        assert lib.ga3c_ddpg_actors_set(h, b"noise_count", wptr, 8) == 0
        word[0] = 0
        assert lib.ga3c_ddpg_actors_get(h, b"noise_count", wptr, 8) == 0 and word[0] == 7
        # destroy, and a second create after it starts from zeros
        assert lib.ga3c_ddpg_envnoise_destroy(h) == 0 and lib.ga3c_ddpg_envnoise_destroy(h) == ESTATE
        nothing_named(h, ESTATE)
        assert lib.ga3c_ddpg_envnoise_create(h, 2, 0) == 0
        assert lib.ga3c_ddpg_actors_get(h, b"noise_x", ptr, 4 * n * A) == 0 and np.all(buf == 0)
        assert lib.ga3c_ddpg_actors_get(h, b"noise_count", wptr, 8) == 0 and word[0] == 0
        # actors_destroy drops it
        assert lib.ga3c_ddpg_actors_destroy(h) == 0
        assert lib.ga3c_ddpg_envnoise_destroy(h) == ESTATE
        assert lib.ga3c_ddpg_actors_create(h, n, 1, 1) == 0
        nothing_named(h, ESTATE)
        assert lib.ga3c_ddpg_envnoise_create(h, 3, 0) == 0                 # left live for the handle's destroy
        # a handle without the noise process has none to give
        assert lib.ga3c_ddpg_actors_create(quiet._h, n, 1, 1) == 0
        assert lib.ga3c_ddpg_envnoise_create(quiet._h, 1, 0) == ESTATE
        assert lib.ga3c_ddpg_envnoise_create(None, 1, 0) == EINVAL and lib.ga3c_ddpg_envnoise_destroy(None) == EINVAL
    finally:
        net.close()
        quiet.close()


def test_the_python_handle_lists_the_names_while_it_has_them():
    net = _net(S, A, max_batch=32, capacity=64)
    try:
        net.actors_create(8, seed=1, batch=1, updates=1)
        assert "noise_x" not in net.ACTOR_FIELDS and "noise_count" not in net.ACTOR_SCALARS
        names = set(net.ACTOR_FIELDS) | set(net.ACTOR_SCALARS)
        for k in names - {"slots"}:                                       # (no train step yet: no draw to read)
            net.actors_get(k)                                             # as before
        net.envnoise_create(5, True)
        assert set(net.ACTOR_FIELDS) | set(net.ACTOR_SCALARS) == names | {"noise_x", "noise_n", "noise_count"}
        assert net.actors_get("noise_x").shape == (8, A) and net.actors_get("noise_count") == 0
        net.envnoise_destroy()
        assert "noise_x" not in net.ACTOR_FIELDS
        net.actors_destroy()
        net.actors_create(8, seed=1, batch=1, updates=1, noise='per_env')
        assert "noise_n" in net.ACTOR_FIELDS
        net.actors_destroy()
        assert "noise_n" not in net.ACTOR_FIELDS
    finally:
        net.close()


# ---- the product line

LINE = ["GAME=Pendulum-v0", "USE_DDPG=True", "TRAINING_MIN_BATCH_SIZE=64", "DEVICE_AGENTS=64", "DEVICE_DDPG=True", "MAX_SECONDS=2"]


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
    assert all(-1.09 * 200 <= float(r) <= -199 for r, _ in records)
    return records


@pytest.mark.timeout(120)
def test_train_script_runs_per_environment_noise(tmp_path):
    _train(tmp_path, "per_env", ["DEVICE_DDPG_NOISE=per_env", "DEVICE_DDPG_NOISE_RESET=True"])


@pytest.mark.timeout(120)
def test_the_line_without_the_key_is_the_shared_line(tmp_path):
    plain, shared = _train(tmp_path, "plain", []), _train(tmp_path, "shared", ["DEVICE_DDPG_NOISE=shared"])
    k = min(len(plain), len(shared))
    assert plain[:k] == shared[:k]
