"""No GPU: the n-step rule of the DDPG device actors (Config.DDPG_NSTEP) as tests/nstep_oracle.py states it.
The delay line that the kernel restates is held to the brute-force per-episode definition on random streams, at n = 1 to
ddpg_actors_oracle's own rows bit for bit, and the Config rules, the ABI names and the Python surface are checked."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ddpg_actors_oracle as do
import device_pendulum_oracle as po
import nstep_oracle as ns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (1, 2, 3, 5, 16)
GAMMA = 0.99


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_row(a, b):
    return all(np.array_equal(_bits(np.asarray(x, np.float32)), _bits(np.asarray(y, np.float32))) for x, y in zip(a, b))


def _stream(rng, dones):
    """Transitions (s, a, r f64, done, s2) with the given done pattern; s of a transition is s2 of the one before."""
    out, s = [], rng.uniform(-1, 1, do.S).astype(np.float32)
    for d in dones:
        s2 = rng.uniform(-1, 1, do.S).astype(np.float32)
        out.append((s, rng.uniform(-2, 2, do.A).astype(np.float32), np.float64(rng.uniform(-1.09, -1.0)), bool(d), s2))
        s = s2
    return out


def _patterns(rng):
    """Done patterns: none; episodes of length 1 on consecutive steps; lengths on both sides of every n; an end on the last
    step; random ones, dense and sparse."""
    T = 70
    yield np.zeros(T, bool)
    d = np.zeros(T, bool)
    d[[3, 4, 5, 6, 20, 21, 40]] = True                       # ends on consecutive steps: episodes of length 1
    yield d
    for length in (1, 2, 3, 4, 5, 6, 15, 16, 17):
        d = np.zeros(T, bool)
        d[length - 1::length] = True
        yield d
    d = np.zeros(T, bool)
    d[-1] = True
    yield d
    for p in (0.05, 0.3, 0.7):
        for _ in range(4):
            yield rng.uniform(size=T) < p


@pytest.mark.parametrize("n", NS)
def test_the_delay_line_is_the_per_episode_definition(n):
    rng = np.random.Generator(np.random.PCG64(100 + n))
    patterns = list(_patterns(rng))
    streams = [_stream(rng, d) for d in patterns]
    T = len(streams[0])
    line = ns.DelayLine(len(streams), n, GAMMA)
    emitted = [[] for _ in streams]
    for c in range(T):
        out = line.push([s[c] for s in streams])
        assert (out is None) == (c < n - 1)
        for i, pair in enumerate(out or []):
            emitted[i].append((c - n + 1,) + pair)             # the row that leaves on step c began at u = c - n + 1
    short = 0
    for stream, got, dones in zip(streams, emitted, patterns):
        want = ns.brute_force(stream, n, GAMMA)
        assert len(got) == len(want) == T - n + 1
        for (u, row, disc), (wu, wrow, wdisc) in zip(got, want):
            assert u == wu and _same_row(row, wrow) and _bits(disc) == _bits(wdisc)
            # what the row is, said once more without either: the horizon ends with the episode
            ahead = np.flatnonzero(dones[u:u + n])
            m = int(ahead[0]) + 1 if ahead.size else n
            assert row[3] == (1.0 if ahead.size else 0.0) and row[4] is stream[u + m - 1][4] and row[0] is stream[u][0]
            assert abs(float(disc) - 0.99 ** m) < 1e-6
            short += m < n
    assert short > 0 or n == 1


def test_the_return_is_summed_in_ascending_order_without_fusing():
    g = ns.gamma64(GAMMA)
    r = [np.float64(-1.0123456789), np.float64(-1.0765432101), np.float64(-1.05)]
    row, disc = ns.nstep_row([(None, None, x, False, None) for x in r], GAMMA)
    assert row[2] == np.float32((0.0 + 1.0 * float(r[0])) + g * float(r[1]) + (g * g) * float(r[2]))
    assert disc == np.float32(g * g * g) and row[3] == 0.0
    row, disc = ns.nstep_row([(None, None, r[0], True, None), (None, None, r[1], False, None)], GAMMA)
    assert row[2] == np.float32(r[0]) and disc == np.float32(GAMMA) and row[3] == 1.0       # nothing across an episode's end


def test_one_step_is_the_actors_oracle_bit_for_bit():
    n_env, seed, steps = 5, 11, 30
    plain, line = do.Actors(n_env, seed), ns.Actors(n_env, seed, 1, GAMMA)
    ring, nring = do.Ring(37), ns.Ring(37, gamma=GAMMA)
    rng = np.random.Generator(np.random.PCG64(5))
    for actors in (plain, line):
        for i, e in enumerate(actors.env):
            e.elapsed = po.TIME_LIMIT - 2 - 3 * i                # episodes end inside the run, on different steps
    records = 0
    for step in range(steps):
        actions = None if step == 0 else rng.uniform(-3.5, 3.5, (n_env, do.A)).astype(np.float32)
        rows, eps, _ = plain.step(actions)
        pairs, neps, _ = line.step(actions)
        assert eps == neps and len(pairs) == len(rows) == (0 if step == 0 else n_env)
        for row, (nrow, disc) in zip(rows, pairs):
            assert _same_row(row, nrow) and _bits(disc) == _bits(np.float32(GAMMA))
        ring.add(rows)
        nring.add([p[0] for p in pairs], [p[1] for p in pairs])
        records += len(eps)
    assert records == n_env and ring.total == nring.total == (steps - 1) * n_env > ring.capacity
    assert np.array_equal(_bits(ring.rows), _bits(nring.rows)) and np.all(nring.disc == np.float32(GAMMA))


def test_silent_steps_and_shortened_rows_over_the_actors():
    n_env, seed, n = 3, 4, 5
    line = ns.Actors(n_env, seed, n, GAMMA)
    line.env[1].elapsed = po.TIME_LIMIT - 8                      # its episode ends on transition 6 (step(None) counts one)
    sizes, dones, discs = [], [], []
    for step in range(14):
        pairs, _, _ = line.step(None if step == 0 else np.zeros((n_env, do.A), np.float32))
        sizes.append(len(pairs))
        if pairs:
            dones.append(float(pairs[1][0][3]))
            discs.append(pairs[1][1])
    assert sizes == [0] * n + [n_env] * (14 - n)                 # step(None) and the n - 1 silent transition steps
    # environment 1's transitions 0..6: rows 0 and 1 see no end, rows 2..6 end with the episode with horizons 5, 4, 3, 2, 1
    g = ns.gamma64(GAMMA)
    assert dones == [0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0]
    assert discs[2:7] == [np.float32(g * g * g * g * g), np.float32(g * g * g * g), np.float32(g * g * g), np.float32(g * g), np.float32(g)]


BASE = dict(GAME='Pendulum-v0', USE_DDPG=True, CONTINUOUS_INPUT=True, DISCRATE_INPUT=False, DEVICE_AGENTS=64, DEVICE_DDPG=True,
            TRAINING_MIN_BATCH_SIZE=64, USE_REPLAY_MEMORY=False, DISCOUNTING=True)
REFUSED = [
    (dict(DDPG_NSTEP=0), "DDPG_NSTEP=0"),
    (dict(DDPG_NSTEP=17), "DDPG_NSTEP=17"),
    (dict(DDPG_NSTEP=-1), "DDPG_NSTEP=-1"),
    (dict(DDPG_NSTEP=2.5), "DDPG_NSTEP=2.5"),
    (dict(DDPG_NSTEP=5, USE_DDPG=False, DEVICE_DDPG=False, DEVICE_AGENTS=0), "needs USE_DDPG"),
    (dict(DDPG_NSTEP=5, DEVICE_DDPG=False, DEVICE_AGENTS=0), "needs DEVICE_DDPG"),
    (dict(DDPG_NSTEP=5, DEVICE_DDPG=False, DEVICE_AGENTS=0), "TIME_MAX"),        # ... and says why
    (dict(DDPG_NSTEP=5, DDPG_FUTURE_REWARD_CALC=False), "DDPG_FUTURE_REWARD_CALC"),
]


@pytest.mark.parametrize("case", REFUSED, ids=["%d_%s" % (i, c[1].split("=")[0].split()[-1]) for i, c in enumerate(REFUSED)])
def test_config_refusals(case, monkeypatch):
    import ga3c_amd  # noqa: F401
    import Config as cfg
    settings, message = case
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert cfg.Config.DDPG_NSTEP == 1
    for k, v in BASE.items():
        monkeypatch.setattr(cfg.Config, k, v)
    for good in (1, 2, 5, 16):                                   # the combination passes at every n
        with monkeypatch.context() as mp:
            mp.setattr(cfg.Config, "DDPG_NSTEP", good)
            cfg.resolve_ddpg()
            cfg.resolve_device_agents()
    for k, v in settings.items():
        monkeypatch.setattr(cfg.Config, k, v)
    with pytest.raises(ValueError, match=re.escape(message)):
        cfg.resolve_ddpg()
        cfg.resolve_device_agents()


def test_a_plain_config_resolves_as_before(monkeypatch):
    import ga3c_amd  # noqa: F401
    import Config as cfg
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for k, v in dict(BASE, DEVICE_DDPG=False, DEVICE_AGENTS=0).items():      # the host path, one-step
        monkeypatch.setattr(cfg.Config, k, v)
    cfg.resolve_ddpg()
    cfg.resolve_device_agents()
    assert cfg.Config.DDPG_NSTEP == 1 and cfg.Config.USE_REPLAY_MEMORY and not cfg.Config.DISCOUNTING
    monkeypatch.setattr(cfg.Config, "USE_DDPG", False)
    before = dict(vars(cfg.Config))
    cfg.resolve_ddpg()
    assert dict(vars(cfg.Config)) == before


def test_argv_sets_the_steps(monkeypatch):
    import ga3c_amd  # noqa: F401
    import GA3C
    from Config import Config
    for k in ("GAME", "USE_DDPG", "CONTINUOUS_INPUT", "DISCRATE_INPUT", "TRAINING_MIN_BATCH_SIZE", "USE_REPLAY_MEMORY", "DISCOUNTING",
              "DEVICE_AGENTS", "DEVICE_DDPG", "DDPG_NSTEP"):
        monkeypatch.setattr(Config, k, getattr(Config, k))       # restored afterwards
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    line = ["GAME=Pendulum-v0", "USE_DDPG=True", "TRAINING_MIN_BATCH_SIZE=64", "DEVICE_AGENTS=64", "DEVICE_DDPG=True"]
    GA3C.apply_argv(line + ["DDPG_NSTEP=5"])
    assert Config.DDPG_NSTEP == 5 and type(Config.DDPG_NSTEP) is int
    with pytest.raises(ValueError, match="DDPG_NSTEP=17"):
        GA3C.apply_argv(line + ["DDPG_NSTEP=17"])


def test_abi_entries():
    import ga3c_amd  # noqa: F401
    import _native as nat
    import NetworkDDPG
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ga3c_abi.h")).read(), flags=re.S)
    lib = nat.hip_lib()
    sig = nat.HIP_SIGNATURES
    for entry in ("create", "destroy", "get", "set"):
        name = "ga3c_ddpg_nstep_" + entry
        assert re.search(r"\bint %s\s*\(ga3c_ddpg\* net" % name, text), name
        assert name in sig and hasattr(lib, name), name
    assert sig["ga3c_ddpg_nstep_create"] == (C.c_int, [C.c_void_p, C.c_int32])
    assert sig["ga3c_ddpg_nstep_destroy"] == (C.c_int, [C.c_void_p])
    assert sig["ga3c_ddpg_nstep_get"] == sig["ga3c_ddpg_nstep_set"] == (C.c_int, [C.c_void_p, nat.f32p, C.c_int64])
    assert re.search(r"int ga3c_ddpg_nstep_create\(ga3c_ddpg\* net, int32_t n\);", text)
    assert re.search(r"int ga3c_ddpg_nstep_get\(ga3c_ddpg\* net, float\* disc, int64_t count\);", text)
    assert re.search(r"int ga3c_ddpg_nstep_set\(ga3c_ddpg\* net, const float\* disc, int64_t count\);", text)
    assert re.search(r"#define GA3C_DDPG_NSTEP_MAX 16\b", text)
    assert C.sizeof(nat.DdpgConfig) == 80                        # attached to a live handle: the config did not grow
    for method in ("nstep_create", "nstep_discounts", "set_nstep_discounts"):
        assert callable(getattr(NetworkDDPG.Network, method)), method
    assert NetworkDDPG.Network.ACTOR_SCALARS["nstep"] is np.int32 and NetworkDDPG.Network.ACTOR_SCALARS["nstep_count"] is np.int64
