"""No GPU: tests/ddpg_task_oracle.py -- the statement the DDPG device actors' kernels are held to under a task --
against ddpg_actors_oracle and nstep_oracle at the fork's task, against EnvironmentPend.Pendulum (gym's Pendulum-v0 restated) at
gym's task, and rule by rule in between; then the Config keys, the ABI entries and what NetworkDDPG asks of the library.

Exact: everything but the rewards against EnvironmentPend.Pendulum, which squares with `**` (pow) where the oracle and the
device multiply: those are held to one spacing of the f64 reward."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import ddpg_actors_oracle as do
import ddpg_task_oracle as to
import device_pendulum_oracle as po
import nstep_oracle as ns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 8642
EPISODE = po.TIME_LIMIT


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _policy(t, i):
    """The stand-in policy: multiples of 0.25 in [-3.5, 3.5], inside the bound, beyond either end and more than a turn beyond."""
    return np.array([0.25 * ((7 * t + 3 * i) % 29 - 14)], np.float32)


def _same_row(a, b):
    return all(_eq(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def _run(actors, steps, n):
    """step(None), then `steps` steps under _policy -> the list of (rows, episodes, outs) per step."""
    out = [actors.step(None)]
    for t in range(steps):
        out.append(actors.step([_policy(t, i) for i in range(n)]))
    return out


def test_the_stand_in_policy_reaches_every_branch():
    a = np.array([_policy(t, i)[0] for t in range(60) for i in range(3)])
    assert a.min() == -3.5 and a.max() == 3.5 and np.all(a * 4 == np.round(a * 4))
    assert (np.abs(a) <= 1).any() and (a > 1).any() and (a < -1).any() and (a > 3).any() and (a < -3).any()


def test_the_forks_task_is_the_actors_oracle_over_three_episodes():
    n, steps = 3, 3 * EPISODE + 5
    mine, theirs = to.Actors(n, SEED, to.FORK), do.Actors(n, SEED)
    episodes = 0
    for (rows, eps, outs), (rows0, eps0, outs0) in zip(_run(mine, steps, n), _run(theirs, steps, n)):
        assert len(rows) == len(rows0) and all(_same_row(a, b) for a, b in zip(rows, rows0))
        assert eps == eps0
        for a, b in zip(outs, outs0):
            assert _eq(np.float64(a["reward"]), np.float64(b["reward"])) and a["done"] == b["done"] == a["terminal"]
        for e, e0 in zip(mine.env, theirs.env):
            assert _eq(e.phys, e0.phys) and _eq(e.obs, e0.obs) and e.elapsed == e0.elapsed and e.rng.draws == e0.rng.draws
        episodes += len(eps)
    assert episodes == 3 * n


def test_the_forks_task_is_the_nstep_oracle():
    n, steps, gamma = 2, 2 * EPISODE + 7, 0.99
    mine, theirs = to.NStepActors(n, SEED, 3, gamma, to.FORK), ns.Actors(n, SEED, 3, gamma)
    emitted = 0
    for (rows, eps, _), (rows0, eps0, _) in zip(_run(mine, steps, n), _run(theirs, steps, n)):
        assert len(rows) == len(rows0) and eps == eps0
        for (row, disc), (row0, disc0) in zip(rows, rows0):
            assert _same_row(row, row0) and _eq(disc, disc0)
        emitted += len(rows)
    assert emitted == n * (steps - 2)


def test_gyms_task_is_the_gym_restatement_over_three_episodes():
    """EnvironmentPend.Pendulum driven with 2 a as gym's user drives it: reset() -> the observation, step -> the observation, the
    reward and the time limit, reset again when it is reached.  The oracle's environment made the two resets and the zero-torque
    first step of the device actors before its first transition; the pendulum is taken through the same."""
    import ga3c_amd  # noqa: F401
    import EnvironmentPend
    n, steps = 2, 3 * EPISODE + 5
    mine = to.Actors(n, SEED, to.GYM)
    pend = [EnvironmentPend.Pendulum(po.ResetRNG(SEED, i)) for i in range(n)]
    obs = []
    for p in pend:
        p.reset()
        p.reset()
        obs.append(np.asarray(p.step(np.zeros(1))[0], np.float32))
    mine.step(None)
    worst, ends, clipped = 0.0, 0, 0
    for t in range(steps):
        actions = [_policy(t, i) for i in range(n)]
        rows, eps, outs = mine.step(actions)
        for i, p in enumerate(pend):
            new_obs, reward, ended = p.step(actions[i].astype(np.float64) * 2.0)
            s, a, r, d, s2 = rows[i]
            assert _eq(s, obs[i]) and _eq(a, actions[i]) and d == 0.0
            assert _eq(s2, np.asarray(new_obs, np.float32))            # physics and observation exact
            assert bool(ended) == outs[i]["done"] and not outs[i]["terminal"]
            want = np.float64(reward)
            assert abs(outs[i]["reward"] - want) <= np.spacing(abs(want)), (t, i)
            worst = max(worst, abs(outs[i]["reward"] - want) / np.spacing(abs(want)))
            assert r == np.float32(outs[i]["reward"])
            clipped += int(abs(actions[i][0]) > 1)
            if ended:
                ends += 1
                obs[i] = np.asarray(p.reset(), np.float32)             # gym: the next episode starts at its reset state
            else:
                obs[i] = np.asarray(new_obs, np.float32)
            assert _eq(mine.env[i].phys, np.asarray(p.state, np.float64)) and _eq(mine.env[i].obs, obs[i])
    assert ends == 3 * n and clipped > steps and worst <= 1.0


def test_clip_is_check_bounds_without_turnaround():
    import ga3c_amd  # noqa: F401
    import EnvironmentPend
    rng = np.random.Generator(np.random.PCG64(3))
    values = np.concatenate([rng.uniform(-6, 6, 2000), [-1.0, 1.0, 0.0, -0.0, np.nextafter(1.0, 2.0), np.nextafter(-1.0, -2.0),
                                                         3.4e38, -3.4e38]]).astype(np.float32)
    for a in values:
        got = to.clip_bounds(a)
        assert _eq(got, EnvironmentPend.check_bounds([np.float64(a)], 1.0, -1.0, False)[0])
        assert _eq(to.bound(to.GYM, a), got) and _eq(to.bound(to.FORK, a), do.check_bounds(a))
        assert -1.0 <= got <= 1.0 and _eq(np.float64(2.0) * got, np.clip(np.float64(a) * 2.0, -2.0, 2.0))    # gym's own clip
    beyond = values[np.abs(values) > 1]
    assert len(beyond) > 1000 and all(abs(to.clip_bounds(a)) == 1.0 for a in beyond)


def test_the_reward_at_the_forks_values_is_the_forks_expression():
    cost = np.random.Generator(np.random.PCG64(4)).uniform(0.0, 17.0, 100000)
    assert _eq(to.reward_of(to.FORK, cost), -cost * 0.005 - 1.0)
    assert _eq(to.reward_of(to.GYM, cost), -cost)
    t = to.Task('wrap', 'terminal', False, 0.1, 0.5)
    assert _eq(to.reward_of(t, cost), -cost * 0.1 + 0.5)
    # ... and through a step: the cost is PendulumEnv.physics's
    for k in range(200):
        phys = np.array([cost[k] - 8.0, cost[k + 200] / 2 - 4.0])
        stepped, c = to.physics_cost(phys, np.float64(cost[k + 400] / 8.5 - 1.0))
        stepped0, r0 = po.PendulumEnv.physics(phys, np.float64(cost[k + 400] / 8.5 - 1.0))
        assert _eq(stepped, stepped0) and _eq(np.float64(to.reward_of(to.FORK, c)), np.float64(r0))


def _ending(task, n=3, start=EPISODE - 4, steps=12):
    """n environments whose episodes end on steps 3 - i of the run -> (actors, per-step outputs)."""
    actors = to.Actors(n, SEED, task)
    actors.step(None)
    for i, e in enumerate(actors.env):
        e.elapsed = start + i
    return actors, [actors.step([_policy(t, i) for i in range(n)]) for t in range(steps)]


def test_truncated_rows_bootstrap_through_the_observation_before_the_reset():
    fork, f = _ending(to.FORK)
    trunc, g = _ending(to.FORK._replace(time_limit='truncate'))
    ends = 0
    for t, ((rows, eps, outs), (rows0, eps0, outs0)) in enumerate(zip(g, f)):
        assert eps == eps0                                             # the records follow `ended`
        for i, (row, row0) in enumerate(zip(rows, rows0)):
            ended = t == 3 - i
            assert outs[i]["done"] == outs0[i]["done"] == ended and outs0[i]["terminal"] == ended and not outs[i]["terminal"]
            assert row[3] == 0.0 and row0[3] == (1.0 if ended else 0.0)
            assert all(_eq(row[k], row0[k]) for k in (0, 1, 2, 4))      # s2: the observation of the physics before the reset
            ends += ended
    assert ends == 3
    for e, e0 in zip(trunc.env, fork.env):                             # the resets drew the same uniforms
        assert _eq(e.phys, e0.phys) and e.rng.draws == e0.rng.draws == 6 and e.elapsed == e0.elapsed


def test_reset_observation_starts_the_next_transition_at_the_reset_state():
    stale, f = _ending(to.FORK)
    fresh, g = _ending(to.FORK._replace(reset_observation=True))
    seen = 0
    for t in range(len(f) - 1):
        for i in range(3):
            row, row0 = g[t][0][i], f[t][0][i]
            nxt, nxt0 = g[t + 1][0][i], f[t + 1][0][i]
            if g[t][2][i]["done"]:
                assert _eq(row[4], row0[4]) and row[3] == row0[3] == 1.0     # the ending row itself is the fork's
                assert _eq(nxt0[0], row0[4])                                  # the fork: the stale observation
                assert not _eq(nxt[0], row[4])
                seen += 1
            elif t < 3 - i:
                assert _same_row(row, row0)
    assert seen == 3
    # four steps: environment 0 has just been reset, and its observation is that of the reset physics, or the stale one
    (again, _), (before, _) = _ending(to.FORK._replace(reset_observation=True), steps=4), _ending(to.FORK, steps=4)
    e, e0 = again.env[0], before.env[0]
    assert e.elapsed == e0.elapsed == 0 and _eq(e.phys, e0.phys)
    assert _eq(e.obs, po.PendulumEnv.observe(e.phys)) and not _eq(e0.obs, po.PendulumEnv.observe(e0.phys))
    assert _eq(g[4][0][0][0], e.obs) and _eq(f[4][0][0][0], e0.obs)      # ... where the next row starts


def test_nstep_rows_across_a_truncated_end():
    """Against the rule stated directly: transition j of an episode of L sums the next min(n, L - j) rewards; under 'truncate' its
    done is 0 and its discount gamma^m all the same."""
    n, gamma, steps = 3, 0.99, 14
    task = to.FORK._replace(time_limit='truncate', reset_observation=True)
    single = to.Actors(1, SEED, task)
    line = to.NStepActors(1, SEED, n, gamma, task)
    for a in (single, line):
        a.step(None)
        a.env[0].elapsed = EPISODE - 6                                  # transitions 0..5 end the first episode
    stream, emitted = [], []
    for t in range(steps):
        rows, _, outs = single.step([_policy(t, 0)])
        stream.append((rows[0], outs[0]))
        emitted += line.step([_policy(t, 0)])[0]
    assert len(emitted) == steps - (n - 1)
    g64, cut = ns.gamma64(gamma), 0
    for u, (row, disc) in enumerate(emitted):
        m = min(n, 6 - u) if u < 6 else n
        R, g = 0.0, 1.0
        for k in range(m):
            R = R + g * float(stream[u + k][1]["reward"])
            g = g * g64
        assert _eq(row[0], stream[u][0][0]) and _eq(row[1], stream[u][0][1])
        assert _eq(row[2], np.float32(R)) and row[3] == 0.0 and _eq(disc, np.float32(g))
        assert _eq(row[4], stream[u + m - 1][0][4])
        cut += m < n
    assert cut == 2
    # the same stream under 'terminal': the cut rows, and only they, are done
    term = to.NStepActors(1, SEED, n, gamma, to.FORK._replace(reset_observation=True))
    term.step(None)
    term.env[0].elapsed = EPISODE - 6
    rows = [r for t in range(steps) for r in term.step([_policy(t, 0)])[0]]
    assert [float(r[0][3]) for r in rows] == [1.0 if 3 <= u < 6 else 0.0 for u in range(len(rows))]
    assert all(_eq(a[1], b[1]) and _eq(a[0][2], b[0][2]) for a, b in zip(rows, emitted))


def test_step_many_is_the_scalar_step():
    rng = np.random.Generator(np.random.PCG64(5))
    phys = np.stack([rng.uniform(-10, 10, 64), rng.uniform(-8, 8, 64)], axis=1)
    action = rng.uniform(-1, 1, 64).astype(np.float32)
    action[:8] = [1.0, -1.0, 1.5, -1.5, 3.25, -3.25, 0.0, 0.999]
    for task in (to.FORK, to.GYM, to.Task('clip', 'terminal', False, 0.1, 0.5)):
        stepped, reward, obs = to.step_many(task, phys, action)
        for i in range(64):
            s, r = to.env_step(task, phys[i], action[i:i + 1])
            assert _eq(stepped[i], s) and _eq(reward[i], np.float64(r)) and _eq(obs[i], po.PendulumEnv.observe(s))
    assert to.gym_return(to.FORK, -230.0, 200) == (-230.0 + 200) / 0.005 and to.gym_return(to.GYM, -900.0, 200) == -900.0


# ---- Config
BASE = dict(GAME='Pendulum-v0', USE_DDPG=True, DEVICE_AGENTS=64, DEVICE_DDPG=True, DEVICE_PENDULUM=False, DEVICE_DDPG_UPDATES=1,
            TRAINING_MIN_BATCH_SIZE=64, REPLAY_BUFFER_SIZE=1000000, PLAY_MODE=False, DYNAMIC_SETTINGS=False,
            DEVICE_AGENT_STEPS=32, DEVICE_DDPG_EVAL_ENVS=0, add_OUnoise=True)
DEFAULTS = dict(DEVICE_DDPG_ACTION_BOUND='wrap', DEVICE_DDPG_TIME_LIMIT='terminal', DEVICE_DDPG_RESET_OBSERVATION=False,
                DEVICE_DDPG_REWARD_SCALE=0.005, DEVICE_DDPG_REWARD_OFFSET=-1.0)
GYM_KEYS = dict(DEVICE_DDPG_ACTION_BOUND='clip', DEVICE_DDPG_TIME_LIMIT='truncate', DEVICE_DDPG_RESET_OBSERVATION=True,
                DEVICE_DDPG_REWARD_SCALE=1.0, DEVICE_DDPG_REWARD_OFFSET=0.0)
OFF = dict(DEVICE_DDPG=False, DEVICE_AGENTS=0)
GATE = [
    (dict(DEVICE_DDPG_ACTION_BOUND='clamp'), "DEVICE_DDPG_ACTION_BOUND="),
    (dict(DEVICE_DDPG_ACTION_BOUND=True), "DEVICE_DDPG_ACTION_BOUND="),
    (dict(DEVICE_DDPG_TIME_LIMIT='truncated'), "DEVICE_DDPG_TIME_LIMIT="),
    (dict(DEVICE_DDPG_TIME_LIMIT=None), "DEVICE_DDPG_TIME_LIMIT="),
    (dict(DEVICE_DDPG_RESET_OBSERVATION=1), "DEVICE_DDPG_RESET_OBSERVATION="),
    (dict(DEVICE_DDPG_RESET_OBSERVATION='True'), "DEVICE_DDPG_RESET_OBSERVATION="),
    (dict(DEVICE_DDPG_REWARD_SCALE=0.0), "DEVICE_DDPG_REWARD_SCALE="),
    (dict(DEVICE_DDPG_REWARD_SCALE=-1.0), "DEVICE_DDPG_REWARD_SCALE="),
    (dict(DEVICE_DDPG_REWARD_SCALE=float('inf')), "DEVICE_DDPG_REWARD_SCALE="),
    (dict(DEVICE_DDPG_REWARD_SCALE=float('nan')), "DEVICE_DDPG_REWARD_SCALE="),
    (dict(DEVICE_DDPG_REWARD_SCALE='1'), "DEVICE_DDPG_REWARD_SCALE="),
    (dict(DEVICE_DDPG_REWARD_SCALE=True), "DEVICE_DDPG_REWARD_SCALE="),
    (dict(DEVICE_DDPG_REWARD_OFFSET=float('nan')), "DEVICE_DDPG_REWARD_OFFSET="),
    (dict(DEVICE_DDPG_REWARD_OFFSET=float('-inf')), "DEVICE_DDPG_REWARD_OFFSET="),
    (dict(DEVICE_DDPG_REWARD_OFFSET=None), "DEVICE_DDPG_REWARD_OFFSET="),
    (dict(OFF, DEVICE_DDPG_ACTION_BOUND='clip'), "DEVICE_DDPG_ACTION_BOUND='clip' needs DEVICE_DDPG "),
    (dict(OFF, DEVICE_DDPG_TIME_LIMIT='truncate'), "DEVICE_DDPG_TIME_LIMIT='truncate' needs DEVICE_DDPG "),
    (dict(OFF, DEVICE_DDPG_RESET_OBSERVATION=True), "DEVICE_DDPG_RESET_OBSERVATION=True needs DEVICE_DDPG "),
    (dict(OFF, DEVICE_DDPG_REWARD_SCALE=1.0), "DEVICE_DDPG_REWARD_SCALE=1.0 needs DEVICE_DDPG "),
    (dict(OFF, DEVICE_DDPG_REWARD_OFFSET=0.0), "DEVICE_DDPG_REWARD_OFFSET=0.0 needs DEVICE_DDPG "),
    (dict(DEVICE_DDPG=False, USE_DDPG=False, GAME='CartPole-v0', DEVICE_AGENTS=8, DEVICE_DDPG_ACTION_BOUND='clip'),
     "DEVICE_DDPG_ACTION_BOUND='clip' needs DEVICE_DDPG "),
    (dict(DEVICE_DDPG=False, USE_DDPG=False, DEVICE_PENDULUM=True, DEVICE_AGENTS=8, DEVICE_DDPG_REWARD_OFFSET=0.0),
     "DEVICE_DDPG_REWARD_OFFSET=0.0 needs DEVICE_DDPG "),
]


@pytest.mark.parametrize("case", GATE, ids=["%s_%d" % (sorted(c[0].items())[-1][0], i) for i, c in enumerate(GATE)])
def test_the_gate(case, monkeypatch):
    import ga3c_amd  # noqa: F401
    import Config as cfg
    settings, message = case
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert all(getattr(cfg.Config, k) == v and type(getattr(cfg.Config, k)) is type(v) for k, v in DEFAULTS.items())
    for k, v in BASE.items():
        monkeypatch.setattr(cfg.Config, k, v)
    cfg.resolve_device_agents()                       # the defaults pass, and so does every option alone and gym's line
    for extra in [{k: v} for k, v in GYM_KEYS.items()] + [GYM_KEYS, dict(DEVICE_DDPG_REWARD_SCALE=1, DEVICE_DDPG_REWARD_OFFSET=0),
                                                          dict(DEVICE_DDPG_REWARD_SCALE=0.1, DEVICE_DDPG_REWARD_OFFSET=0.5)]:
        with monkeypatch.context() as mp:
            for k, v in extra.items():
                mp.setattr(cfg.Config, k, v)
            cfg.resolve_device_agents()
    for k, v in settings.items():
        monkeypatch.setattr(cfg.Config, k, v)
    with pytest.raises(ValueError, match=re.escape(message)):
        cfg.resolve_device_agents()


def test_the_defaults_leave_the_resolvers_alone(monkeypatch):
    import ga3c_amd  # noqa: F401
    import Config as cfg
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert all(getattr(cfg.Config, k) == v for k, v in DEFAULTS.items())
    assert dict(cfg.DEVICE_DDPG_TASK_DEFAULTS) == DEFAULTS
    before = dict(vars(cfg.Config))
    cfg.resolve_action_space()
    cfg.resolve_ddpg()
    cfg.resolve_device_agents()
    assert dict(vars(cfg.Config)) == before
    # ... and under DEVICE_DDPG, at the defaults and with gym's line
    for k, v in dict(BASE, CONTINUOUS_INPUT=True, DISCRATE_INPUT=False).items():
        monkeypatch.setattr(cfg.Config, k, v)
    for k in ("USE_REPLAY_MEMORY", "DISCOUNTING"):
        monkeypatch.setattr(cfg.Config, k, getattr(cfg.Config, k))
    cfg.resolve_ddpg()
    held = dict(vars(cfg.Config))
    cfg.resolve_device_agents()
    assert dict(vars(cfg.Config)) == held
    for k, v in GYM_KEYS.items():
        monkeypatch.setattr(cfg.Config, k, v)
    held = dict(vars(cfg.Config))
    cfg.resolve_device_agents()
    assert dict(vars(cfg.Config)) == held


def test_a_default_of_another_type_is_a_default_in_both_places(monkeypatch):
    """-1 for -1.0, numpy's 0.005 for 0.005: the resolver without DEVICE_DDPG and Network.__init__ make one comparison."""
    import ga3c_amd  # noqa: F401
    import Config as cfg
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    same = dict(DEVICE_DDPG_REWARD_OFFSET=-1, DEVICE_DDPG_REWARD_SCALE=np.float64(0.005), DEVICE_DDPG_RESET_OBSERVATION=0)
    for k, v in same.items():
        monkeypatch.setattr(cfg.Config, k, v)
    cfg.resolve_device_agents()                       # DEVICE_AGENTS = 0: nothing asks for DEVICE_DDPG
    net, asked = _made(monkeypatch)
    assert [a[0] for a in asked] == ["ga3c_ddpg_create"] and net.task is None


def test_the_command_line_sets_the_keys(monkeypatch):
    import ga3c_amd  # noqa: F401
    import Config as cfg
    import GA3C
    for k, v in dict(BASE, CONTINUOUS_INPUT=True, DISCRATE_INPUT=False, **DEFAULTS).items():
        monkeypatch.setattr(cfg.Config, k, v)
    for k in ("USE_REPLAY_MEMORY", "DISCOUNTING"):
        monkeypatch.setattr(cfg.Config, k, getattr(cfg.Config, k))
    GA3C.apply_argv(["DEVICE_DDPG_ACTION_BOUND=clip", "DEVICE_DDPG_TIME_LIMIT=truncate", "DEVICE_DDPG_RESET_OBSERVATION=True",
                     "DEVICE_DDPG_REWARD_SCALE=1", "DEVICE_DDPG_REWARD_OFFSET=0"])
    assert {k: getattr(cfg.Config, k) for k in GYM_KEYS} == GYM_KEYS
    assert all(type(getattr(cfg.Config, k)) is type(v) for k, v in GYM_KEYS.items())
    cfg.resolve_device_agents()


# ---- the ABI and the Python handle
def test_abi_entries():
    import ga3c_amd  # noqa: F401
    import _native as nat
    import NetworkDDPG
    text = open(os.path.join(ROOT, "include", "ga3c_abi.h")).read()
    lib = nat.hip_lib()
    for entry in ("create", "destroy", "info"):
        name = "ga3c_ddpg_task_" + entry
        assert re.search(r"\bint %s\s*\(ga3c_ddpg\* net" % name, text), name
        assert name in nat.HIP_SIGNATURES and hasattr(lib, name), name
    sig = nat.HIP_SIGNATURES
    assert sig["ga3c_ddpg_task_create"] == (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double])
    assert sig["ga3c_ddpg_task_destroy"] == (C.c_int, [C.c_void_p])
    assert sig["ga3c_ddpg_task_info"] == (C.c_int, [C.c_void_p, nat.i32p, nat.i32p, nat.i32p, nat.f64p, nat.f64p])
    assert re.search(r"int ga3c_ddpg_task_create\(ga3c_ddpg\* net, int32_t bound, int32_t time_limit, int32_t reset_observation,\s*"
                     r"double reward_scale,\s*double reward_offset\);", text)
    for name, value in (("WRAP", 0), ("CLIP", 1), ("TERMINAL", 0), ("TRUNCATE", 1)):
        assert re.search(r"#define GA3C_DDPG_TASK_%s %d\b" % (name, value), text), name
    assert C.sizeof(nat.DdpgConfig) == 80             # attached to a live handle, no flag bit: the config did not grow
    # the existing signatures are what they were
    assert sig["ga3c_ddpg_actors_create"] == (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64])
    assert sig["ga3c_ddpg_eval_create"] == (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int32])
    assert sig["ga3c_ddpg_eval_run"] == (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, nat.f64p])
    for method in ("task_create", "task_info", "task_destroy"):
        assert callable(getattr(NetworkDDPG.Network, method)), method
    assert NetworkDDPG.FORK_TASK == tuple(to.FORK) == tuple(DEFAULTS.values())


class _Recorder:
    """Stands in for the library: every entry answers 0 and is written down."""

    def __init__(self):
        self.asked = []

    def __getattr__(self, name):
        def entry(*args):
            self.asked.append((name,) + tuple(a for a in args[1:] if isinstance(a, (int, float))))
            return 0
        return entry


def _made(monkeypatch, **keys):
    import ga3c_amd  # noqa: F401
    from Config import Config
    import NetworkDDPG
    import _native as nat
    lib = _Recorder()
    monkeypatch.setattr(nat, "hip_lib", lambda: lib)
    for k, v in keys.items():
        monkeypatch.setattr(Config, k, v)
    net = NetworkDDPG.Network("gpu:0", "task_cpu", 1, (3,), max_batch=16, predict_lanes=1, replay_capacity=64)
    net._h = None                                     # nothing to destroy
    return net, [a for a in lib.asked if a[0] not in ("ga3c_ddpg_set_param",)]


def test_network_init_asks_for_nothing_new_at_the_defaults(monkeypatch):
    net, asked = _made(monkeypatch)
    assert [a[0] for a in asked] == ["ga3c_ddpg_create"] and net.task is None
    with monkeypatch.context() as mp:                 # after nstep_create
        net, asked = _made(mp, DDPG_NSTEP=3, DEVICE_DDPG_ACTION_BOUND='clip')
        assert [a[0] for a in asked] == ["ga3c_ddpg_create", "ga3c_ddpg_nstep_create", "ga3c_ddpg_task_create", "ga3c_ddpg_task_info"]
        assert asked[2] == ("ga3c_ddpg_task_create", 1, 0, 0, 0.005, -1.0)
    for key, value, want in (("DEVICE_DDPG_TIME_LIMIT", 'truncate', (0, 1, 0, 0.005, -1.0)),
                             ("DEVICE_DDPG_RESET_OBSERVATION", True, (0, 0, 1, 0.005, -1.0)),
                             ("DEVICE_DDPG_REWARD_SCALE", 1.0, (0, 0, 0, 1.0, -1.0)),
                             ("DEVICE_DDPG_REWARD_OFFSET", 0.0, (0, 0, 0, 0.005, 0.0))):
        with monkeypatch.context() as mp:             # each option alone
            _, asked = _made(mp, **{key: value})
            assert asked[1] == ("ga3c_ddpg_task_create",) + want, key
    net, asked = _made(monkeypatch, **GYM_KEYS)
    assert asked[1] == ("ga3c_ddpg_task_create", 1, 1, 1, 1.0, 0.0) and net.task is not None
    with pytest.raises(ValueError, match="bound="):
        net.task_create('clamp', 'terminal', False, 1.0, 0.0)
    with pytest.raises(ValueError, match="time_limit="):
        net.task_create('clip', 'never', False, 1.0, 0.0)
    net.task_destroy()
    assert net.task is None


def test_log_eval_undoes_the_tasks_reward(tmp_path, monkeypatch):
    import threading
    import ga3c_amd  # noqa: F401
    import NetworkDDPG
    monkeypatch.chdir(tmp_path)
    totals = np.array([-230.5, -201.25, -260.0])
    mean = float(totals.mean())

    def logged(name, **attrs):
        model = types.SimpleNamespace(model_name=name, _log_lock=threading.Lock(), **attrs)
        NetworkDDPG.Network.log_eval(model, 7000, totals, 200)
        return open(os.path.join("logs", name, "eval.csv")).read()

    today = "%d,%d,%d,%.17g,%.17g,%.17g,%.17g\n" % (7000, 3, 200, mean, totals.min(), totals.max(), (mean + 200) / 0.005)
    assert logged("no_attribute") == today             # a stand-in model that borrows the method
    assert logged("no_task", task=None) == today
    assert logged("fork", task=NetworkDDPG.FORK_TASK) == today
    line = logged("gym", task=('clip', 'truncate', True, 1.0, 0.0))
    assert line.endswith(",%.17g\n" % mean)
    line = logged("scaled", task=('wrap', 'terminal', False, 0.1, 0.5))
    assert line.endswith(",%.17g\n" % ((mean - 200 * 0.5) / 0.1)) and float(line.split(",")[-1]) == to.gym_return(
        to.Task('wrap', 'terminal', False, 0.1, 0.5), mean, 200)
