"""Per-environment exploration noise of the DDPG device actors (Config.DEVICE_DDPG_NOISE) on the CPU:
tests/envnoise_oracle.py -- the statement the device is held to -- for what its draws must be as random numbers, for its step
against ddpg_oracle.ou_step and for its reset rule; the Config rules; the ABI entries; and what NetworkDDPG.Network asks of the
library when its actors are created.

The statistical bounds are 5 standard errors of the estimated quantity for independent standard normals: with M draws the mean
has standard error 1 / sqrt(M), the variance sqrt(2 / M) (the variance of n^2 is 2), and the mean product of two independent
sequences 1 / sqrt(M) (the variance of a product of two independent standard normals is 1)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ddpg_oracle as o
import device_agents_oracle as ao
import envnoise_oracle as eo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENVS, PREDICTIONS, SEED = 4096, 64, 12347


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def table():
    """n f32 [ENVS][PREDICTIONS] and the smallest u1, computed once and left unchanged."""
    cols, low = [], 1.0
    for c in range(PREDICTIONS):
        u1, _ = eo.uniforms(SEED, ENVS, c, 1)
        low = min(low, float(u1.min()))
        cols.append(eo.draws(SEED, ENVS, c, 1)[:, 0])
    n = np.stack(cols, axis=1)
    n.setflags(write=False)
    return n, low


def test_the_draws_are_standard_normal(table):
    n, low = table
    assert n.dtype == np.float32 and n.shape == (ENVS, PREDICTIONS) and np.all(np.isfinite(n))
    M = n.size
    v = n.astype(np.float64)
    assert abs(v.mean()) <= 5.0 / np.sqrt(M)
    assert abs(v.var() - 1.0) <= 5.0 * np.sqrt(2.0 / M)
    assert 0.0 < low <= 1.0                                  # u1 = 1 - u with u in [0, 1): ln u1 is finite
    assert float(np.min(1.0 - ao.uniform(SEED, np.arange(ENVS), 0))) >= 2.0 ** -53


def test_no_two_environments_share_a_sequence_and_neighbours_do_not_correlate(table):
    n, _ = table
    assert len(np.unique(_bits(n), axis=0)) == ENVS
    v = n.astype(np.float64)
    pairs = v[:-1] * v[1:]
    assert abs(pairs.mean()) <= 5.0 / np.sqrt(pairs.size)
    # ... and neither do an environment's own consecutive predictions
    own = v[:, :-1] * v[:, 1:]
    assert abs(own.mean()) <= 5.0 / np.sqrt(own.size)
    # another seed, other sequences
    assert not np.array_equal(eo.draws(SEED + 1, 64, 0, 1), eo.draws(SEED, 64, 0, 1))


def test_the_draw_number_is_c_A_plus_j_and_an_environment_does_not_depend_on_how_many_there_are():
    two = np.stack([eo.draws(SEED, 33, c, 2) for c in range(6)], axis=1)              # [33][6][2]
    one = np.stack([eo.draws(SEED, 33, k, 1)[:, 0] for k in range(12)], axis=1)        # [33][12]
    assert _eq(two.reshape(33, 12), one)
    assert _eq(eo.draws(SEED, 300, 5, 1)[:33], eo.draws(SEED, 33, 5, 1))
    # written out for one cell: environment 7, prediction 3, action 1 of 2
    k = 3 * 2 + 1
    u1, u2 = 1.0 - float(ao.uniform(SEED, 7, 2 * k)), float(ao.uniform(SEED, 7, 2 * k + 1))
    want = np.float32(np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2))
    assert _eq(eo.draws(SEED, 33, 3, 2)[7, 1], want)


def test_the_step_is_ou_step_on_the_same_draws_rounded_to_f32():
    rng = np.random.Generator(np.random.PCG64(5))
    x = rng.normal(0.0, 0.4, size=(300, 1)).astype(np.float32)
    n = eo.draws(SEED, 300, 9, 1)
    cfg = eo.f32_config()
    assert cfg["sigma"] == np.float64(np.float32(0.3)) != 0.3 and cfg["dt"] == np.float64(np.float32(1e-2))
    got = eo.step(x, n)
    assert got.dtype == np.float32
    assert _eq(got, o.ou_step(x.astype(np.float64), n.astype(np.float64), **cfg).astype(np.float32))
    # the expression, operand by operand, in f64
    x64, n64 = x.astype(np.float64), n.astype(np.float64)
    assert _eq(got, (x64 + cfg["theta"] * (0.0 - x64) * cfg["dt"] + cfg["sigma"] * np.sqrt(cfg["dt"]) * n64).astype(np.float32))
    # other constants are taken as their f32 values too
    assert _eq(eo.step(x, n, sigma=0.7, theta=0.4, dt=0.05),
               o.ou_step(x64, n64, **eo.f32_config(0.7, 0.4, 0.05)).astype(np.float32))
    # the state of a handle: zeros, then step after step on draws c = 0, 1, ..
    z = eo.EnvNoise(17, 2, SEED)
    assert np.all(z.x == 0) and z.count == 0
    x = np.zeros((17, 2), np.float32)
    for c in range(5):
        x = eo.step(x, eo.draws(SEED, 17, c, 2))
        assert _eq(z.predict(), x) and z.count == c + 1 and _eq(z.n, eo.draws(SEED, 17, c, 2))


def test_the_reset_starts_from_zero_after_a_done_and_nowhere_else():
    rng = np.random.Generator(np.random.PCG64(6))
    x = (rng.normal(0.0, 0.4, size=(40, 1)).astype(np.float32) + np.float32(0.01))
    assert np.all(x != 0)
    done = np.zeros(40, np.int32)
    done[[0, 7, 39]] = 1
    prev = eo.x_prev(x, done, True)
    assert np.all(prev[done != 0] == 0.0) and _eq(prev[done == 0], x.astype(np.float64)[done == 0])
    assert _eq(eo.x_prev(x, done, False), x.astype(np.float64))
    n = eo.draws(SEED, 40, 2, 1)
    with_reset, without = eo.step(x, n, done, True), eo.step(x, n, done, False)
    assert _eq(with_reset[done != 0], eo.step(np.zeros((3, 1), np.float32), n[done != 0]))
    assert _eq(with_reset[done == 0], without[done == 0]) and not np.array_equal(with_reset[done != 0], without[done != 0])
    # over a run: environment i's episode ends on step 3 + i
    z, ref = eo.EnvNoise(4, 1, SEED, reset=True), eo.EnvNoise(4, 1, SEED, reset=False)
    for t in range(10):
        done = (np.arange(4) + 3 == t - 1).astype(np.int32)          # the step before this prediction ended the episode
        before = z.x.copy()
        got, plain = z.predict(done), ref.predict(done)
        start = np.where(done[:, None] != 0, np.float32(0.0), before)
        assert _eq(got, eo.step(start, z.n))
        if t < 4:
            assert _eq(got, plain)                                   # nothing has ended yet: the two agree


BASE = dict(GAME='Pendulum-v0', USE_DDPG=True, DEVICE_AGENTS=64, DEVICE_DDPG=True, DEVICE_PENDULUM=False, DEVICE_DDPG_UPDATES=1,
            TRAINING_MIN_BATCH_SIZE=64, REPLAY_BUFFER_SIZE=1000000, PLAY_MODE=False, DYNAMIC_SETTINGS=False,
            DEVICE_AGENT_STEPS=32, DEVICE_DDPG_EVAL_ENVS=0, add_OUnoise=True, DEVICE_DDPG_NOISE='per_env',
            DEVICE_DDPG_NOISE_RESET=False)
GATE = [
    (dict(DEVICE_DDPG_NOISE='each'), "DEVICE_DDPG_NOISE="),
    (dict(DEVICE_DDPG_NOISE=True), "DEVICE_DDPG_NOISE="),
    (dict(DEVICE_DDPG_NOISE=None), "DEVICE_DDPG_NOISE="),
    (dict(add_OUnoise=False), "add_OUnoise"),
    (dict(add_OUnoise=''), "add_OUnoise"),
    (dict(DEVICE_DDPG_NOISE_RESET=1), "DEVICE_DDPG_NOISE_RESET"),
    (dict(DEVICE_DDPG_NOISE_RESET='True'), "DEVICE_DDPG_NOISE_RESET"),
    (dict(DEVICE_DDPG_NOISE='shared', DEVICE_DDPG_NOISE_RESET=None), "DEVICE_DDPG_NOISE_RESET"),
    (dict(DEVICE_DDPG=False, DEVICE_AGENTS=0), "DEVICE_DDPG_NOISE='per_env' needs DEVICE_DDPG "),
    (dict(DEVICE_DDPG=False, USE_DDPG=False, GAME='CartPole-v0', DEVICE_AGENTS=8), "DEVICE_DDPG_NOISE='per_env' needs DEVICE_DDPG "),
    (dict(DEVICE_DDPG=False, USE_DDPG=False, DEVICE_PENDULUM=True, DEVICE_AGENTS=8), "DEVICE_DDPG_NOISE='per_env' needs DEVICE_DDPG "),
]


@pytest.mark.parametrize("case", GATE, ids=["%s_%d" % (sorted(c[0].items())[0][0], i) for i, c in enumerate(GATE)])
def test_the_gate(case, monkeypatch):
    import ga3c_amd  # noqa: F401
    import Config as cfg
    settings, message = case
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert cfg.Config.DEVICE_DDPG_NOISE == 'shared' and cfg.Config.DEVICE_DDPG_NOISE_RESET is False
    for k, v in BASE.items():
        monkeypatch.setattr(cfg.Config, k, v)
    cfg.resolve_device_agents()                       # the combination passes
    for extra in (dict(DEVICE_DDPG_NOISE_RESET=True), dict(DEVICE_DDPG_NOISE='shared'),
                  dict(DEVICE_DDPG_NOISE='shared', add_OUnoise=False), dict(DEVICE_AGENTS=1), dict(DEVICE_AGENTS=4096)):
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
    assert cfg.Config.DEVICE_DDPG_NOISE == 'shared' and cfg.Config.DEVICE_DDPG_NOISE_RESET is False
    before = dict(vars(cfg.Config))
    cfg.resolve_action_space()
    cfg.resolve_ddpg()
    cfg.resolve_device_agents()
    assert dict(vars(cfg.Config)) == before
    # ... and under DEVICE_DDPG with the two keys at their defaults
    for k, v in dict(BASE, DEVICE_DDPG_NOISE='shared', CONTINUOUS_INPUT=True, DISCRATE_INPUT=False).items():
        monkeypatch.setattr(cfg.Config, k, v)
    for k in ("USE_REPLAY_MEMORY", "DISCOUNTING"):
        monkeypatch.setattr(cfg.Config, k, getattr(cfg.Config, k))
    cfg.resolve_ddpg()
    held = dict(vars(cfg.Config))
    cfg.resolve_device_agents()
    assert dict(vars(cfg.Config)) == held
    # 'shared' without the device regime asks for nothing
    for k, v in dict(DEVICE_DDPG=False, DEVICE_AGENTS=0).items():
        monkeypatch.setattr(cfg.Config, k, v)
    cfg.resolve_device_agents()


def test_abi_entries():
    import ga3c_amd  # noqa: F401
    import _native as nat
    import NetworkDDPG
    text = open(os.path.join(ROOT, "include", "ga3c_abi.h")).read()
    lib = nat.hip_lib()
    for entry in ("create", "destroy"):
        name = "ga3c_ddpg_envnoise_" + entry
        assert re.search(r"\bint %s\s*\(ga3c_ddpg\* net" % name, text), name
        assert name in nat.HIP_SIGNATURES and hasattr(lib, name), name
    sig = nat.HIP_SIGNATURES
    assert sig["ga3c_ddpg_envnoise_create"] == (C.c_int, [C.c_void_p, C.c_int64, C.c_int32])
    assert sig["ga3c_ddpg_envnoise_destroy"] == sig["ga3c_ddpg_actors_destroy"]
    assert re.search(r"int ga3c_ddpg_envnoise_create\(ga3c_ddpg\* net, int64_t seed, int32_t reset_on_done\);", text)
    assert re.search(r"int ga3c_ddpg_envnoise_destroy\(ga3c_ddpg\* net\);", text)
    for name in ('"noise_x"', '"noise_n"', '"noise_count"'):
        assert name in text, name
    assert C.sizeof(nat.DdpgConfig) == 80             # attached to a live handle, no flag bit: the config did not grow
    assert "GA3C_DDPG_ENVNOISE" not in text and "GA3C_DDPG_NOISE_PER" not in text
    # the existing signatures are what they were
    assert sig["ga3c_ddpg_actors_create"] == (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64])
    assert sig["ga3c_ddpg_actors_run"] == (C.c_int, [C.c_void_p, C.c_int32, C.c_float, C.c_float, C.c_int32, C.c_int32, nat.f32p,
                                                     nat.i64p, nat.f32p])
    Network = NetworkDDPG.Network
    for method in ("envnoise_create", "envnoise_destroy"):
        assert callable(getattr(Network, method)), method
    assert Network.NOISE_FIELDS == {"noise_x": (np.float32, "A"), "noise_n": (np.float32, "A")}
    assert Network.NOISE_SCALARS == {"noise_count": np.int64}


def test_actors_create_asks_for_the_noise_the_config_names(monkeypatch):
    import ga3c_amd  # noqa: F401
    from Config import Config
    import NetworkDDPG

    class Stub(NetworkDDPG.Network):
        max_batch = 64

        def __init__(self):
            self.asked = []

        def _call(self, entry, *args):
            self.asked.append((entry,) + tuple(a for a in args if isinstance(a, (int, float))))

        def close(self):
            pass

    def created(**kw):
        net = Stub()
        net.actors_create(8, **kw)
        return net, [a for a in net.asked if a[0] != "actors_set"]

    monkeypatch.setattr(Config, "RANDOM_SEED", 500)
    shared = dict(Stub.ACTOR_FIELDS), dict(Stub.ACTOR_SCALARS)
    net, asked = created()
    assert asked == [("actors_create", 8, 1, 500)]                   # the defaults: nothing new is asked for
    assert "noise_x" not in net.ACTOR_FIELDS and "noise_count" not in net.ACTOR_SCALARS
    net, asked = created(noise='per_env')
    assert asked == [("actors_create", 8, 1, 500), ("envnoise_create", 502, 0)]      # + 1 is the evaluation's seed
    assert net.ACTOR_FIELDS == dict(shared[0], **Stub.NOISE_FIELDS) and net.ACTOR_SCALARS == dict(shared[1], **Stub.NOISE_SCALARS)
    assert (dict(Stub.ACTOR_FIELDS), dict(Stub.ACTOR_SCALARS)) == shared             # the handle's, not every handle's
    net.actors_destroy()
    assert net.ACTOR_FIELDS == shared[0] and net.ACTOR_SCALARS == shared[1]
    net, asked = created(noise='per_env', noise_seed=9, noise_reset=True)
    assert asked[1] == ("envnoise_create", 9, 1)
    net.envnoise_destroy()
    assert net.asked[-1] == ("envnoise_destroy",) and "noise_x" not in net.ACTOR_FIELDS
    monkeypatch.setattr(Config, "DEVICE_DDPG_NOISE", 'per_env')
    monkeypatch.setattr(Config, "DEVICE_DDPG_NOISE_RESET", True)
    net, asked = created()
    assert asked[1] == ("envnoise_create", 502, 1)
    net, asked = created(noise='shared')
    assert len(asked) == 1
    with pytest.raises(ValueError, match="noise="):
        created(noise='each')
