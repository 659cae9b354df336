"""PopArt on the DDPG handle's critic (Config.DDPG_POPART) on the CPU: tests/popart_oracle.py -- the statement the
device is held to -- against tests/ddpg_oracle.py and torch autograd; the kernel's mixed form (f32 storage, f64 update, f32
constants) at its fixed point and over a long run; the Config rules; the ABI entries."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ddpg_oracle as o
import popart_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR = 3e-4


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _case(S, A, B, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    online, target = o.random_params(S, A, rng, stats=True), o.random_params(S, A, rng, stats=True)
    batch = (rng.uniform(-1.5, 1.5, (B, S)), rng.uniform(-1, 1, (B, A)), rng.uniform(-1, 0, B),
             (rng.uniform(size=B) < 0.25).astype(np.float64), rng.uniform(-1.5, 1.5, (B, S)))
    return online, target, batch


@pytest.mark.parametrize("cfg", [dict(), dict(critic_rmsprop=False, clip=40.0), dict(future=False)], ids=["rmsprop", "adam-clip", "y=r"])
def test_a_float64_step_at_beta_zero_is_the_paired_step_exactly(cfg):
    online, target, batch = _case(3, 1, 17, 5)
    noise = np.array([0.05])
    a = o.new_state(online, target, cfg.get("critic_rmsprop", True))
    b = po.new_state(online, target, cfg.get("critic_rmsprop", True))
    for _ in range(3):
        wa = o.train_step(a, *batch, LR, noise, form="paired", **cfg)
        wb = po.train_step(b, *batch, LR, noise, beta=0.0, **cfg)
        for k in ("y", "q", "dq", "g", "a_out"):
            assert _eq(wa[k], wb[k]), k
        assert _eq(wb["yn"], wb["y"]) and wa["q_max"] == wb["q_max"] and wa["q_avg"] == wb["q_avg"]
    assert (b["mu"], b["nu"], b["step"]) == (0.0, 1.0, 3)
    for part in ("online", "target", "slot_a", "slot_b"):
        for k in a[part]:
            assert _eq(a[part][k], b[part][k]), (part, k)


@pytest.mark.parametrize("mu,nu,beta", [(0.0, 1.0, 1.0), (-100.0, 10009.0, 0.3), (-3.0, 9.5, 3e-4)])
def test_a_statistics_jump_preserves_the_outputs_of_both_critics_in_float64(mu, nu, beta):
    """sigma' n' + mu' = sigma n + mu to 1e-12 (relative to the returns' size), online and target, after one float64 step at
    learning rate 0 with targets near -100."""
    online, target, batch = _case(7, 3, 33, 9)
    s, a, r, done, s2 = batch
    r = 100.0 * r - 50.0
    st = po.new_state(online, target, mu=mu, nu=nu)
    sigma = po.sigma_of(mu, nu)
    before = [sigma * o.critic_forward(P, s, a)["q"][:, 0] + mu for P in (st["online"], st["target"])]
    out = po.train_step(st, s, a, r, done, s2, 0.0, beta=beta, stop_after=3)
    assert (st["mu"], st["nu"]) != (mu, nu) and out["sigma"] == po.sigma_of(st["mu"], st["nu"])
    for P, want in zip((st["online"], st["target"]), before):
        got = out["sigma"] * o.critic_forward(P, s, a)["q"][:, 0] + st["mu"]
        assert np.max(np.abs(got - want)) <= 1e-12 * max(1.0, np.max(np.abs(want)))
    # the normalised targets have the statistics' moments when the statistics are the batch's (beta = 1)
    if beta == 1.0:
        assert abs(out["yn"].mean()) <= 1e-9 and abs(np.mean(out["yn"] ** 2) - 1.0) <= 1e-9


def test_the_critics_gradient_is_autograd_of_the_normalised_loss():
    """d/dtheta mean((n - yn)^2) by torch autograd on the float64 critic, against the oracle's critic_grads on yn."""
    torch = pytest.importorskip("torch")
    online, target, batch = _case(3, 1, 17, 11)
    s, a, r, done, s2 = batch
    st = po.new_state(online, target, mu=-2.0, nu=6.0)
    out = po.train_step(st, s, a, 10.0 * r, done, s2, 0.0, beta=0.5, stop_after=3)
    O = st["online"]                                        # after the rescale; the learning rate was 0
    P = {k: torch.tensor(O[k], dtype=torch.float64, requires_grad=True) for k in o.CRITIC_TRAINABLE}
    stat = {k: torch.tensor(O[k]) for k in ("critic_norm1/moving_mean", "critic_norm1/moving_variance")}
    x, act, yn = torch.tensor(s), torch.tensor(a), torch.tensor(out["yn"])
    h1 = x @ P["critic_fc1/W"] + P["critic_fc1/b"]
    n1 = P["critic_norm1/gamma"] * (h1 - stat["critic_norm1/moving_mean"]) / torch.sqrt(stat["critic_norm1/moving_variance"] + o.BN_EPS) \
        + P["critic_norm1/beta"]
    t = torch.relu(n1) @ P["critic_fc2/W"] + act @ P["critic_norm2/W"] + P["critic_norm2/b"]
    n = (torch.relu(t) @ P["critic_output/W"] + P["critic_output/b"])[:, 0]
    ((n - yn) ** 2).mean().backward()
    for k in o.CRITIC_TRAINABLE:
        want = np.zeros_like(O[k]) if P[k].grad is None else P[k].grad.numpy()
        got = np.asarray(out["critic_grads"][k]).reshape(want.shape)
        assert np.max(np.abs(got - want)) <= 1e-12 * max(1.0, np.max(np.abs(want))), k


def test_the_mixed_form_at_beta_zero_reproduces_its_inputs_bit_for_bit():
    rng = np.random.default_rng(3)
    W, b = rng.uniform(-0.3, 0.3, (300, 1)).astype(np.float32), rng.uniform(-0.3, 0.3, 1).astype(np.float32)
    y = rng.uniform(-120, -80, 33).astype(np.float32)
    # fresh statistics: every factor is exactly 1 or 0
    mu1, nu1 = po.update_mixed(0.0, 1.0, y, 0.0)
    assert _eq(mu1, np.float32(0.0)) and _eq(nu1, np.float32(1.0))
    ratio, shift, muf, isig, sigma, sigma1 = po.constants(0.0, 1.0, mu1, nu1)
    assert (float(ratio), float(shift), float(muf), float(isig), sigma, sigma1) == (1.0, 0.0, 0.0, 1.0, 1.0, 1.0)
    W1, b1 = po.rescale(W, b, ratio, shift)
    assert _eq(W1, W) and _eq(b1, b) and _eq(po.normalise(y, muf, isig), y)
    # ... and any stored statistics stay what they are, with the weights
    mu, nu = np.float32(-99.75), np.float32(9959.5)
    mu1, nu1 = po.update_mixed(mu, nu, y, 0.0)
    assert _eq(mu1, mu) and _eq(nu1, nu)
    ratio, shift, _, _, _, _ = po.constants(mu, nu, mu1, nu1)
    W1, b1 = po.rescale(W, b, ratio, shift)
    assert float(ratio) == 1.0 and float(shift) == 0.0 and _eq(W1, W) and _eq(b1, b)
    # the exact fmaf against f64, where one f64 rounding cannot differ: products of small integers
    assert _eq(po.fmaf32(np.float32(3.0), np.float32(5.0), np.float32(0.25)), np.float32(15.25))
    # ... a product far below the sum's spacing, the tie 1 + 2^-24 (to even), and just above it
    assert _eq(po.fmaf32(np.float32(2.0 ** -30), np.float32(2.0 ** -30), np.float32(1.0)), np.float32(1.0))
    assert _eq(po.fmaf32(np.float32(2.0 ** -24), np.float32(1.0), np.float32(1.0)), np.float32(1.0))
    assert _eq(po.fmaf32(np.float32(2.0 ** -24 + 2.0 ** -47), np.float32(1.0), np.float32(1.0)), np.float32(1.0 + 2.0 ** -23))


def test_two_thousand_mixed_updates_at_minus_one_hundred_keep_sigma_inside_the_clamps():
    """Targets -100 + N(0, 3), 64 rows a step, at Config's beta.  nu - mu^2 is the difference of two numbers near 10^4 whose f32
    storage is good to 5e-4 each: sigma stays finite, inside the clamps, and the head's return-scale output moves by at most
    3.1e-5 of its size per update in float32."""
    import ga3c_amd  # noqa: F401
    from Config import Config
    rng = np.random.default_rng(17)
    W, b = rng.uniform(-0.003, 0.003, (300, 1)).astype(np.float32), np.zeros(1, np.float32)
    c2 = np.maximum(rng.normal(0.0, 1.0, (64, 300)), 0.0).astype(np.float32)
    mu, nu = np.float32(0.0), np.float32(1.0)
    lo, hi = po.bounds32(Config.DDPG_POPART_SIGMA_MIN, Config.DDPG_POPART_SIGMA_MAX)
    worst, sigmas = 0.0, []
    for _ in range(2000):
        y = (-100.0 + rng.normal(0.0, 3.0, 64)).astype(np.float32)
        before, after, (W, b, mu, nu) = po.preserved((W, b), c2, mu, nu, y, Config.DDPG_POPART_BETA,
                                                     Config.DDPG_POPART_SIGMA_MIN, Config.DDPG_POPART_SIGMA_MAX)
        sigma = po.sigma_of(mu, nu, lo, hi)
        assert np.isfinite(sigma) and lo <= sigma <= hi and np.all(np.isfinite(W)) and np.isfinite(b).all()
        sigmas.append(sigma)
        worst = max(worst, float(np.max(np.abs(after - before))) / max(1.0, float(np.max(np.abs(before)))))
    print("sigma after 2000 updates %.6g (smallest %.6g, largest %.6g), mu %.6g; largest move of the output %.3e"
          % (sigmas[-1], min(sigmas), max(sigmas), float(mu), worst))
    assert lo < min(sigmas) and max(sigmas) < hi            # the clamps were never what held it
    assert worst <= 3.1e-5


BASE = dict(GAME='Pendulum-v0', USE_DDPG=True, TRAINING_MIN_BATCH_SIZE=64, REPLAY_BUFFER_SIZE=100000, CONTINUOUS_INPUT=True,
            DISCRATE_INPUT=False, DDPG_CRITIC_LOSS='paired', DDPG_POPART=True, DDPG_TWIN=False, DDPG_DISTRIBUTIONAL=False,
            DUAL_RMSPROP=False, FRONTEND='host')
GATE = [
    (dict(USE_DDPG=False), "DDPG_POPART needs USE_DDPG"),
    (dict(DDPG_CRITIC_LOSS='fork'), "DDPG_POPART with DDPG_CRITIC_LOSS='fork'"),
    (dict(DDPG_TWIN=True), "DDPG_TWIN"),
    (dict(DDPG_DISTRIBUTIONAL=True), "DDPG_DISTRIBUTIONAL"),
    (dict(DDPG_POPART_BETA=-0.1), "DDPG_POPART_BETA=-0.1"),
    (dict(DDPG_POPART_BETA=1.5), "DDPG_POPART_BETA=1.5"),
    (dict(DDPG_POPART_BETA=float("nan")), "DDPG_POPART_BETA=nan"),
    (dict(DDPG_POPART_BETA=True), "DDPG_POPART_BETA=True"),
    (dict(DDPG_POPART_SIGMA_MIN=0.0), "DDPG_POPART_SIGMA_MIN / _MAX = 0.0 / "),
    (dict(DDPG_POPART_SIGMA_MIN=2.0, DDPG_POPART_SIGMA_MAX=1.0), "DDPG_POPART_SIGMA_MIN / _MAX = 2.0 / 1.0"),
    (dict(DDPG_POPART_SIGMA_MAX=float("inf")), "DDPG_POPART_SIGMA_MIN / _MAX = "),
    (dict(DDPG_POPART_SIGMA_MIN=float("nan")), "DDPG_POPART_SIGMA_MIN / _MAX = nan"),
]


@pytest.mark.parametrize("case", GATE, ids=["%s_%d" % (sorted(c[0].items())[0][0], i) for i, c in enumerate(GATE)])
def test_the_config_rules_and_their_messages(case, monkeypatch):
    import ga3c_amd  # noqa: F401
    import Config as cfg
    settings, message = case
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    K = cfg.Config
    assert (K.DDPG_POPART, K.DDPG_POPART_BETA, K.DDPG_POPART_SIGMA_MIN, K.DDPG_POPART_SIGMA_MAX) == (False, 3e-4, 1e-4, 1e6)
    for k, v in BASE.items():
        monkeypatch.setattr(K, k, v)
    for k in ("USE_REPLAY_MEMORY", "DISCOUNTING"):
        monkeypatch.setattr(K, k, getattr(K, k))
    cfg.resolve_ddpg()                                    # the combination passes, alone and with priorities
    with monkeypatch.context() as mp:
        mp.setattr(K, "PRIORITIZED_REPLAY", True)
        cfg.resolve_ddpg()
    for k, v in settings.items():
        monkeypatch.setattr(K, k, v)
    with pytest.raises(ValueError, match=re.escape(message)):
        cfg.resolve_ddpg()
    if "DDPG_TWIN" in settings or "DDPG_DISTRIBUTIONAL" in settings:
        with pytest.raises(ValueError, match="DDPG_POPART"):
            cfg.resolve_ddpg()


def test_the_defaults_leave_the_resolver_alone(monkeypatch):
    import ga3c_amd  # noqa: F401
    import Config as cfg
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    before = dict(vars(cfg.Config))
    cfg.resolve_action_space()
    cfg.resolve_ddpg()
    assert dict(vars(cfg.Config)) == before
    # bad numbers are not looked at while the feature is off
    for k, v in dict(BASE, DDPG_POPART=False, DDPG_POPART_BETA=7.0, DDPG_POPART_SIGMA_MIN=-1.0).items():
        monkeypatch.setattr(cfg.Config, k, v)
    for k in ("USE_REPLAY_MEMORY", "DISCOUNTING"):
        monkeypatch.setattr(cfg.Config, k, getattr(cfg.Config, k))
    cfg.resolve_ddpg()


def test_abi_entries():
    import ga3c_amd  # noqa: F401
    import _native as nat
    import NetworkDDPG
    text = open(os.path.join(ROOT, "include", "ga3c_abi.h")).read()
    lib = nat.hip_lib()
    for entry in ("create", "destroy", "info"):
        name = "ga3c_ddpg_popart_" + entry
        assert re.search(r"\bint %s\s*\(ga3c_ddpg\* net" % name, text), name
        assert name in nat.HIP_SIGNATURES and hasattr(lib, name), name
    sig = nat.HIP_SIGNATURES
    assert sig["ga3c_ddpg_popart_create"] == (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_float])
    assert sig["ga3c_ddpg_popart_destroy"] == sig["ga3c_ddpg_twin_destroy"]
    assert sig["ga3c_ddpg_popart_info"] == (C.c_int, [C.c_void_p, nat.f32p, nat.f32p, nat.f32p, nat.f32p])
    assert re.search(r"int ga3c_ddpg_popart_create\(ga3c_ddpg\* net, float beta, float sigma_min, float sigma_max\);", text)
    assert re.search(r"int ga3c_ddpg_popart_destroy\(ga3c_ddpg\* net\);", text)
    assert re.search(r"int ga3c_ddpg_popart_info\(ga3c_ddpg\* net, float\* beta, float\* mu, float\* nu, float\* sigma\);", text)
    for name in ('"yn"', "critic_popart/mu", "critic_popart/nu"):
        assert name in text, name
    assert C.sizeof(nat.DdpgConfig) == 80             # attached to a live handle, no flag bit: the config did not grow
    assert "GA3C_DDPG_POPART" not in text
    assert callable(NetworkDDPG.Network.popart_info)
    plain, pop = NetworkDDPG.param_shapes(3, 1), NetworkDDPG.param_shapes(3, 1, popart=True)
    assert len(plain) == 20 and {k: v for k, v in pop.items() if k in plain} == plain
    assert {k: pop[k] for k in pop if k not in plain} == {"critic_popart/mu": (1,), "critic_popart/nu": (1,)}
