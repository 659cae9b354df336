"""-m gpu: the DDPG handle's soft actor-critic step (ga3c_ddpg_soft_create, Config.DDPG_SOFT) against its f64
statement (tests/sac_oracle.py).

Tolerances are tests/test_gpu_ddpg.py's: 1e-4 x max(1, max|want|) on rows, 1e-5 on weights, slots and log_alpha after steps,
tests/closeness.py's relative error per gradient tensor, 1e-6 absolute for the draws against numpy's restatement (log, sqrt and
cos are the device library's).  The oracle is fed the draws the device made (fetched "s_eps2", "s_eps").  The rows of the cases
that differentiate through relu units are chosen by tests/sac_cases.py, whose docstring has the rule and the learning rates;
tests/test_sac_cpu.py holds that choice to its cap of 4 B candidates without a GPU.  Forward rows (y, q, logp) are continuous in
every pre-activation and need no choice of rows."""
import numpy as np
import pytest

import ddpg_oracle as o
import sac_cases as sc
import sac_oracle as so
import td3_oracle as t3
from test_gpu_ddpg import WTOL, _check, _net

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -4
SOFT_FETCH = dict(s_eps2="A", s_a2="A", s_logp2=1, s_vt=1, s_mu="A", s_ls="A", s_eps="A", s_u="A", s_logp=1, s_q1=1, s_q2=1)


def _snet(S, A, delay=1, max_batch=160, capacity=512, **kw):
    kw.setdefault("DDPG_CRITIC_LOSS", "paired")
    return _net(S, A, max_batch=max_batch, capacity=capacity, DDPG_TWIN=True, DDPG_SOFT=True, DDPG_POLICY_DELAY=delay,
                RANDOM_SEED=sc.SEED, **kw)


def _load(net, online, target):
    for k in so.ALL_VARS:
        net.set_variable_value(k, online[k], 0)
        net.set_variable_value(k, target[k], 1)


def _args(b):
    return b[0], b[2], b[1], b[4], b[3]          # Network.train's order: x, y_r, a, x2, done


def _f32(P):
    return {k: v.astype(np.float32) for k, v in P.items()}


def _draws(net, t, B, A, policy=True):
    """-> the device's draws of step t (eps2, eps), held to numpy's."""
    want2, want1 = so.step_draws(sc.SOFT_SEED, t, B, A)
    got = []
    for name, want in (("s_eps2", want2),) + ((("s_eps", want1),) if policy else ()):
        eps = net.fetch(name, B * A).reshape(B, A)
        err = float(np.max(np.abs(eps.astype(np.float64) - want)))
        print("%s: max |device - numpy| %.3e, largest |draw| %.2f" % (name, err, float(np.max(np.abs(want)))))
        assert err <= 1e-6
        got.append(eps)
    return got if policy else (got[0], want1)


def _snapshot(net, names=so.TRAINABLE):
    return {(k, w): net.get_variable_value(k, w) for k in names for w in (0, 1, 2, 3)}


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


# ---- 1. one policy step, every row

def _grad_floors(S, A, B, online, target, batch, eps2, eps, out, w32, lr):
    """What replaces closeness.py's e32 where rel_err(g32, g64) is a SINGLE draw of the rounding error (test_gpu_td3._single_draws
    has the argument; everything here is the oracle's).  -> {tensor name: floor}.
      * critic_output/b and critic2_output/b are one element, the sum of dq over the rows: closeness.e32_of_row_sum.
      * actor_output/b is 2A elements, each the sum of a column of "do" over the rows: the largest e32_of_row_sum of a column.
      * At B = 1 every tensor is one row's dq (or do) times factors without cancellation: the f32 cost of q, y and do is taken from
        64 rows drawn like the candidates under the draws of place 0, E_q + E_y over |q - y| of the row, and E_do over max|do|."""
    import closeness as cl
    floors = {}
    for tag, dq in (("critic_", "dq"), ("critic2_", "dq2")):
        if B > 1:
            floors[tag + "output/b"] = cl.e32_of_row_sum(w32[dq], out[dq])
    if B > 1:
        cols = [cl.e32_of_row_sum(w32["do"][:, j], out["do"][:, j]) for j in range(2 * A) if np.any(out["do"][:, j])]
        floors["actor_output/b"] = max(cols)
    if B == 1:
        rng = np.random.Generator(np.random.PCG64(7))
        rows = sc.candidates(S, A, 64, rng)
        e2, e1 = np.repeat(eps2[:1], 64, axis=0), np.repeat(eps[:1], 64, axis=0)
        y64 = so.targets(online, target, *sc.f64((rows[4], rows[2], rows[3])), 0.99, e2)["y"]
        y32 = so.targets(_f32(online), _f32(target), rows[4], rows[2], rows[3], np.float32(0.99), e2)["y"]
        e_y = float(np.max(np.abs(y32.astype(np.float64) - y64)))
        for tag, view, q_name in (("critic_", lambda P: P, "q"), ("critic2_", t3.critic2, "q2")):
            q64 = o.critic_forward(view(online), *sc.f64((rows[0], rows[1])))["q"][:, 0]
            q32 = o.critic_forward(view(_f32(online)), rows[0], rows[1])["q"][:, 0]
            e_dq = (float(np.max(np.abs(q32 - q64))) + e_y) / abs(float(out[q_name][0] - out["y"][0]))
            floors.update({tag + k[len("critic_"):]: e_dq for k in o.CRITIC_TRAINABLE})
        st64, st32 = so.new_state(online, target), so.new_state(_f32(online), _f32(target))
        e_do = 0.0
        for i in range(64):                      # one row at a time: B = 1 is the 1 / B of "do"
            one = tuple(c[i:i + 1] for c in rows)
            d64 = so.policy_grads(st64["online"], np.asarray(one[0], np.float64), e1[i:i + 1], -float(A))["do"]
            d32 = so.policy_grads(st32["online"], one[0], e1[i:i + 1], np.float32(-A))["do"]
            e_do = max(e_do, float(np.max(np.abs(d32 - d64))))
        floors.update({k: e_do / float(np.max(np.abs(out["do"]))) for k in o.ACTOR_TRAINABLE})
    return floors


def _policy_step(net, online, target, batch, lr, S, A, B, grads="relative"):
    """compute(stop_after = 4) on a loaded handle at step 0 and delay 1 against the oracle -> (out, oracle state)."""
    import closeness as cl
    q_max, q_avg = net.compute(*_args(batch), 4, noise=False)
    eps2, eps = _draws(net, 1, B, A)
    st = so.new_state(online, target)
    out = so.train_step(st, *sc.f64(batch), lr, policy_delay=1, eps2=eps2, eps=eps, stop_after=4)
    w32 = so.train_step(so.new_state(_f32(online), _f32(target)), *batch, np.float32(lr), policy_delay=1, eps2=eps2, eps=eps,
                        stop_after=4, gamma=np.float32(0.99), target_entropy=np.float32(-A))
    _check("q_max", [q_max], [out["q_max"]])
    _check("q_avg", [q_avg], [out["q_avg"]])
    f1, f2, fa = out["critic_fwd"], out["critic2_fwd"], out["fwd"]
    rows = [("y", out["y"]), ("qt", out["qt"]), ("qt1", out["qt1"]), ("qt2", out["qt2"]), ("s_a2", out["a2"]),
            ("s_logp2", out["logp2"]), ("s_vt", out["vt"]),
            ("q", out["q"]), ("dq", out["dq"]), ("c_xh1", f1["xh1"]), ("c_c1", f1["c1"]), ("c_c2", f1["c2"]), ("c_dt", f1["dt"]),
            ("c_dn1", f1["dn1"]), ("q2", out["q2"]), ("dq2", out["dq2"]), ("c2_xh1", f2["xh1"]), ("c2_c1", f2["c1"]),
            ("c2_c2", f2["c2"]), ("c2_dt", f2["dt"]), ("c2_dn1", f2["dn1"]),
            ("s_mu", fa["mu"]), ("s_ls", fa["ls"]), ("s_u", fa["u"]), ("a_noisy", fa["a"]), ("s_logp", fa["logp"]),
            ("s_q1", out["pq1"]), ("s_q2", out["pq2"]), ("g", out["g"]), ("do", out["do"]),
            ("a_xh1", fa["xh1"]), ("a_a1", fa["a1"]), ("a_xh2", fa["xh2"]), ("a_a2", fa["a2"]), ("a_dn2", fa["dn2"]), ("a_dn1", fa["dn1"])]
    for name, want in rows:
        _check(name, net.fetch(name, np.size(want)), want)
    assert np.array_equal(net.fetch("qt", B), np.minimum(net.fetch("qt1", B), net.fetch("qt2", B)))
    sel = net.fetch("s_q2", B) < net.fetch("s_q1", B)
    assert np.array_equal(sel, out["sel"]), "the device selects the oracle's critic on every row"
    failed = []
    floors = _grad_floors(S, A, B, online, target, batch, eps2, eps, out, w32, lr) if grads == "relative" else {}
    tensors = [(pre + k[len("critic_"):], out[tag][k], w32[tag][k]) for pre, tag in (("critic_", "critic_grads"), ("critic2_", "critic2_grads"))
               for k in o.CRITIC_TRAINABLE]
    tensors += [(k, out["actor_grads"][k], w32["actor_grads"][k]) for k in o.ACTOR_TRAINABLE]
    for name, want, want32 in tensors:
        got = net.get_variable_value(name, 4)
        _check("grad " + name, got, want)
        if grads == "relative" and np.any(want):
            assert want32.dtype == np.float32
            e32 = max(cl.rel_err(want32, want), floors.get(name, 0.0))
            err = cl.report("sac S=%d A=%d B=%d" % (S, A, B), "grad " + name, got, want, e32, cl.bound(e32))
            if not err <= cl.bound(e32):
                failed.append((name, err, cl.bound(e32)))
    _check("grad " + so.LOG_ALPHA, net.get_variable_value(so.LOG_ALPHA, 4), [out["dlog_alpha"]])
    assert not failed, failed
    assert abs(net.soft_info()[2] - out["mean_logp"]) <= 1e-4 * max(1.0, abs(out["mean_logp"]))
    assert net.get_global_step() == 0
    return out, st


@pytest.mark.parametrize("S,A,B", sc.EVERY_ROW)
def test_one_policy_step_every_row_and_gradient(S, A, B):
    online, target, batch, _ = sc.every_row_case(S, A, B)
    net = _snet(S, A)
    try:
        net.learning_rate = sc.ROWS_LR
        _load(net, online, target)
        assert len(net.get_variables_names()) == 39
        _policy_step(net, online, target, batch, sc.ROWS_LR, S, A, B)
    finally:
        net.close()


# ---- 2. off a policy step nothing of the actor, the temperature or the targets moves

def test_a_step_off_the_policy_delay_leaves_actor_temperature_and_targets_alone():
    S, A, B = 7, 3, 33
    rng = np.random.Generator(np.random.PCG64(21))
    online, target = so.random_params(S, A, rng), so.random_params(S, A, rng)
    net = _snet(S, A, delay=2)
    try:
        _load(net, online, target)
        before = {(k, w): net.get_variable_value(k, w) for k in o.ACTOR_TRAINABLE + (so.LOG_ALPHA,) for w in (0, 2, 3)}
        before.update({(k, 1): net.get_variable_value(k, 1) for k in so.ALL_VARS})
        critics = {k: net.get_variable_value(k, 0) for k in ("critic_fc1/W", "critic2_fc1/W")}
        net.train(*_args(sc.candidates(S, A, B, rng)), noise=False)            # t = 1
        assert all(np.array_equal(v, net.get_variable_value(k, w)) for (k, w), v in before.items())
        assert not any(np.array_equal(v, net.get_variable_value(k, 0)) for k, v in critics.items()), "both critics step"
        net.train(*_args(sc.candidates(S, A, B, rng)), noise=False)            # t = 2: a policy step
        moved = [kw for kw, v in before.items() if not np.array_equal(v, net.get_variable_value(*kw))]
        assert (so.LOG_ALPHA, 0) in moved and ("actor_fc1/W", 0) in moved and ("critic2_fc1/W", 1) in moved
        assert (so.LOG_ALPHA, 1) not in moved, "log_alpha's target copy is the value given at create"
    finally:
        net.close()


# ---- 3. three production steps

@pytest.mark.parametrize("way,delay", sc.STEP_CASES)
def test_three_production_steps(way, delay):
    from test_gpu_td3 import _AdamCondition
    S, A = sc.STEPS_SHAPE
    B, cfg, kw = sc.STEPS_B, sc.STEP_WAYS[way], sc.steps_kw(way)
    online, target, st, rng = sc.steps_case(way, delay)
    adam = None
    if not cfg.get("RMSPROP", True):
        adam = _AdamCondition(st, so.new_state(_f32(online), _f32(target), critic_rmsprop=False))
    net = _snet(S, A, delay=delay, critic_lr=sc.STEPS_CRITIC_LR, **cfg)
    try:
        _load(net, online, target)
        for step in range(1, sc.STEPS + 1):
            b, _ = sc.select(st, sc.candidates(S, A, 4 * B, rng), B, delay, **kw)
            q_max, q_avg = net.train(*_args(b), noise=False)
            policy = step % delay == 0
            eps2, eps = _draws(net, step, B, A, policy)
            if adam:
                adam.before()
            out = so.train_step(st, *sc.f64(b), sc.LR, policy_delay=delay, eps2=eps2, eps=eps, **kw)
            if adam:
                kw32 = dict(kw, gamma=np.float32(0.99), target_entropy=np.float32(-A))
                adam.after(out, so.train_step(adam.st32, *b, np.float32(sc.LR), policy_delay=delay, eps2=eps2, eps=eps, **kw32),
                           sc.STEPS_CRITIC_LR * sc.LR, step)
            assert out["policy"] == policy
            _check("step %d q_max" % step, [q_max], [out["q_max"]])
            _check("step %d q_avg" % step, [q_avg], [out["q_avg"]])
            _check("step %d y" % step, net.fetch("y", B), out["y"])
        assert net.get_global_step() == sc.STEPS == st["step"]
        for k in so.ALL_VARS:
            if adam and k in adam.shaky:
                adam.check(k, net.get_variable_value(k, 0), st["online"][k], sc.STEPS_CRITIC_LR * sc.LR)
            else:
                _check("online " + k, net.get_variable_value(k, 0), st["online"][k], WTOL)
            _check("target " + k, net.get_variable_value(k, 1), st["target"][k], WTOL)
        for k in so.TRAINABLE:
            _check("slot a " + k, net.get_variable_value(k, 2), st["slot_a"][k], WTOL)
            _check("slot b " + k, net.get_variable_value(k, 3), st["slot_b"][k], WTOL)
        assert not np.array_equal(st["online"][so.LOG_ALPHA], online[so.LOG_ALPHA]), "the temperature moved"
        la = net.soft_info()[0]
        assert abs(la - st["online"][so.LOG_ALPHA][0]) <= WTOL
    finally:
        net.close()


# ---- 4. saturation

def test_saturated_means_and_clamped_log_stds():
    S, A, B = 7, 5, 17
    online, target, batch, _ = sc.saturation_case(S, A, B)
    net = _snet(S, A)
    try:
        net.learning_rate = sc.ROWS_LR
        _load(net, online, target)
        out, _ = _policy_step(net, online, target, batch, sc.ROWS_LR, S, A, B)
        do = net.fetch("do", B * 2 * A).reshape(B, 2 * A)
        ls, u, logp = net.fetch("s_ls", B * A).reshape(B, A), net.fetch("s_u", B * A).reshape(B, A), net.fetch("s_logp", B)
        assert np.array_equal(ls, np.tile(np.float32([2.0, 2.0, -20.0, -20.0, 0.0]), (B, 1)))
        assert not do[:, A:2 * A - 1].any(), "the gradient to a clamped ls is exactly zero"
        assert do[:, 2 * A - 1].all() and np.all(np.isfinite(do)) and np.all(np.isfinite(logp))
        assert np.all(np.isfinite(net.fetch("y", B))) and np.all(np.isfinite(net.fetch("s_logp2", B)))
        print("largest |u| %.2f; entries of a at exactly +-1: %d of %d" % (float(np.max(np.abs(u))),
              int((np.abs(net.fetch("a_noisy", B * A)) == 1.0).sum()), B * A))
        assert np.max(np.abs(u)) > 9.0
        for k in o.ACTOR_TRAINABLE:
            assert np.all(np.isfinite(net.get_variable_value(k, 4))), k
    finally:
        net.close()


# ---- 5. selection

@pytest.mark.parametrize("shift,second", [(10.0, False), (-10.0, True)], ids=["critic1", "critic2"])
def test_the_smaller_critic_gives_the_action_gradient(shift, second):
    S, A, B = 7, 3, 17
    online, target, batch, _ = sc.selection_case(shift, S, A, B)
    net = _snet(S, A)
    try:
        net.learning_rate = sc.ROWS_LR
        _load(net, online, target)
        out, st = _policy_step(net, online, target, batch, sc.ROWS_LR, S, A, B, grads="rows")
        assert np.all(out["sel"] == second)
        q1, q2 = net.fetch("s_q1", B), net.fetch("s_q2", B)
        assert np.all((q2 < q1) == second)
        _check("g is that critic's dq/da", net.fetch("g", B * A), out["g2"] if second else out["g1"])
        assert np.max(np.abs(out["g1"] - out["g2"])) > 1e-3, "the two critics' gradients differ"
    finally:
        net.close()


# ---- 6. predictions

def test_predict_modes_and_the_prediction_count():
    S, A, B = 7, 3, 17
    rng = np.random.Generator(np.random.PCG64(61))
    online, target = so.random_params(S, A, rng, stats=True), so.random_params(S, A, rng, stats=True)
    x = rng.uniform(-1.5, 1.5, (B, S)).astype(np.float32)
    nets = [_snet(S, A) for _ in range(2)]
    try:
        for net in nets:
            _load(net, online, target)
        net = nets[0]
        assert net.soft_info()[3] == 0
        _check("NONE", net.predict(x, noise=False), so.mean_action(online, x))
        given = np.float32([0.5, -1.25, 2.0])
        _check("GIVEN", net.predict(x, noise=given), so.sample(online, x, np.tile(given, (B, 1)))["a"])
        assert net.soft_info()[3] == 0, "only predictions that draw their own noise count"
        for c in range(3):
            got = [n.predict(x) for n in nets]
            assert np.array_equal(got[0], got[1]), "two handles of one seed draw the same"
            _check("OWN %d" % c, got[0], so.sample(online, x, so.predict_draws(sc.SOFT_SEED, c, B, A))["a"])
            assert net.soft_info()[3] == c + 1
        assert not np.array_equal(net.predict(x), got[0])
        assert np.all(np.abs(net.predict(x)) <= 1.0)
    finally:
        for net in nets:
            net.close()


# ---- 7. device actors and evaluation episodes

@pytest.mark.parametrize("task", [None, ("clip", "truncate", True, 1.0, 0.0)], ids=["plain", "task"])
def test_device_actors_sample_per_environment_and_evaluation_acts_by_the_mean(task):
    import ddpg_actors_oracle as do
    S, A, n, steps = do.S, do.A, 33, 4
    rng = np.random.Generator(np.random.PCG64(71))
    online, target = so.random_params(S, A, rng, stats=True), so.random_params(S, A, rng, stats=True)
    net = _snet(S, A, max_batch=64, capacity=400)
    try:
        _load(net, online, target)
        if task:
            net.task_create(*task)
        net.actors_create(n, seed=5, updates=1, batch=16, draw_seed=24680)
        assert net.actors_run(1, train=False) == (n, 0, 0, 0)                  # step(None): no prediction, no draw
        assert net.soft_info()[3] == 0
        for c in range(steps):
            obs = net.actors_get("obs").reshape(n, S).copy()
            net.actors_run(1, train=False)
            eps, action = net.actors_get("soft_eps").reshape(n, A), net.actors_get("action").reshape(n, A)
            want = so.predict_draws(sc.SOFT_SEED, c, n, A)
            assert float(np.max(np.abs(eps.astype(np.float64) - want))) <= 1e-6 and net.soft_info()[3] == c + 1
            _check("actions of step %d" % c, action, so.sample(online, obs, eps)["a"])
            for i in (0, 16, n - 1):                                            # the ring row of environment i holds them
                s_row, a_row = net.replay_get(c * n + i)[:2]
                assert np.array_equal(s_row, obs[i]) and np.array_equal(a_row, action[i])
        assert len({float(v) for v in eps.reshape(-1)}) == n * A, "every environment draws its own"
        # evaluation episodes: bit-equal to stepwise predictions without noise
        net.eval_create(17, seed=9, trace=True)
        net.eval_run(steps=6)
        tobs, tact = net.eval_get("trace_obs"), net.eval_get("trace_action")
        for t in range(6):
            assert np.array_equal(net.predict(tobs[:, t], noise=False).reshape(-1), tact[:, t]), t
        _check("evaluation acts by tanh(mu)", tact[:, 0], so.mean_action(online, tobs[:, 0])[:, 0])
    finally:
        net.close()


# ---- 8. priorities and n-step returns: the forward rows of one step each

def test_prioritized_soft_step():
    S, A, n, B = 3, 1, 128, 33
    rng = np.random.Generator(np.random.PCG64(81))
    online, target = so.random_params(S, A, rng), so.random_params(S, A, rng)
    ring = sc.candidates(S, A, n, rng)
    net = _snet(S, A, capacity=n, PRIORITIZED_REPLAY=True, REPLAY_BUFFER_RANDOM_SEED=sc.SEED)
    try:
        net.learning_rate = sc.ROWS_LR
        _load(net, online, target)
        assert net.replay_add(*ring) == (n, n)
        net.set_priorities(np.random.default_rng(5).uniform(0.01, 2, n).astype(np.float32), 2.0)
        net.replay_beta = 0.4
        net.train_prioritized(B, noise=False)
        slots, w = net.last_slots, net.fetch("per_w", B)
        eps2, eps = _draws(net, 1, B, A)
        st = so.new_state(online, target)
        out = so.train_step(st, *sc.f64(tuple(c[slots] for c in ring)), sc.ROWS_LR, policy_delay=1, eps2=eps2, eps=eps,
                            per_w=w.astype(np.float64), stop_after=4)
        for name, key in (("y", "y"), ("qt", "qt"), ("s_logp2", "logp2"), ("s_vt", "vt"), ("q", "q"), ("dq", "dq"), ("q2", "q2"),
                          ("dq2", "dq2"), ("s_q1", "pq1"), ("s_q2", "pq2")):
            _check(name, net.fetch(name, B), out[key])
        _check("s_logp", net.fetch("s_logp", B), out["fwd"]["logp"])
        assert np.array_equal(net.fetch("per_td", B), np.abs(net.fetch("y", B) - net.fetch("q", B)))
        assert net.get_global_step() == 1
    finally:
        net.close()


def test_nstep_soft_step_reads_the_rows_discounts():
    S, A, n, B = 3, 1, 64, 17
    rng = np.random.Generator(np.random.PCG64(82))
    online, target = so.random_params(S, A, rng), so.random_params(S, A, rng)
    ring = sc.candidates(S, A, n, rng)
    disc = (0.99 ** rng.integers(1, 4, n)).astype(np.float32)
    slots = rng.permutation(n)[:B].astype(np.int32)
    net = _snet(S, A, capacity=n)
    try:
        net.learning_rate = sc.ROWS_LR
        net.nstep_create(3)
        _load(net, online, target)
        assert net.replay_add(*ring) == (n, n)
        net.set_nstep_discounts(disc)
        net.train_replay(slots, noise=False)
        eps2, eps = _draws(net, 1, B, A)
        assert np.array_equal(net.fetch("disc", B), disc[slots])
        out = so.train_step(so.new_state(online, target), *sc.f64(tuple(c[slots] for c in ring)), sc.ROWS_LR, policy_delay=1,
                            eps2=eps2, eps=eps, disc=disc[slots].astype(np.float64), stop_after=4)
        for name, key in (("y", "y"), ("qt", "qt"), ("s_vt", "vt"), ("q", "q"), ("dq", "dq")):
            _check(name, net.fetch(name, B), out[key])
        plain = so.targets(online, target, *sc.f64((ring[4][slots], ring[2][slots], ring[3][slots])), 0.99, eps2)["y"]
        assert np.max(np.abs(plain - out["y"])) > 1e-3, "the discounts matter"
    finally:
        net.close()


# ---- 9. checkpoints and refusals

def test_checkpoint_round_trip_resume_and_cross_refusals(tmp_path):
    S, A, B = 3, 1, 17
    rng = np.random.Generator(np.random.PCG64(91))
    online, target = so.random_params(S, A, rng), so.random_params(S, A, rng)
    batches = [sc.candidates(S, A, B, rng) for _ in range(4)]
    path, twin_path = str(tmp_path / "sac.npz"), str(tmp_path / "td3.npz")
    net = _snet(S, A, delay=1)
    try:
        _load(net, online, target)
        for b in batches[:2]:
            net.train(*_args(b), noise=False)
        net._lib.ga3c_ddpg_save(net._h, path.encode())
        two = _snapshot(net)
        net.train(*_args(batches[2]), noise=False)                # Adam's step 3
        three = _snapshot(net)
        with np.load(path) as z:
            names = set(z.files)
            assert int(z["step"]) == 2 and z["actor_output/W:0"].shape == (300, 2 * A)
            for k in ("actor_soft/log_alpha:0", "actor_soft/log_alpha/Adam:0", "actor_soft/log_alpha/Adam_1:0", "soft_config",
                      "critic2_fc1/W:0", "actor_output/b/Adam:0"):
                assert k in names, k
            assert np.array_equal(z["soft_config"], np.float32([-A, -20.0, 2.0])) and z["soft_config"].dtype == np.float32
            assert np.array_equal(z["actor_soft/log_alpha:0"], two[(so.LOG_ALPHA, 0)])
    finally:
        net.close()
    from test_gpu_td3 import _tnet
    fresh, twin, other = _snet(S, A, delay=1), _tnet(S, A, delay=1), _snet(S, A, delay=1, DDPG_SOFT_LOG_STD_MAX=1.0)
    try:
        fresh.load_file(path)
        assert fresh.get_global_step() == 2 and _same(two, _snapshot(fresh))
        fresh.train(*_args(batches[2]), noise=False)              # resumed: the step and its draws are the uninterrupted run's
        assert _same(three, _snapshot(fresh))
        twin.train(*_args(batches[0]), noise=False)
        twin._lib.ga3c_ddpg_save(twin._h, twin_path.encode())
        before_f, before_t, before_o = _snapshot(fresh), _snapshot(twin, t3.TRAINABLE), _snapshot(other)
        assert fresh._lib.ga3c_ddpg_load(fresh._h, twin_path.encode()) == ESTATE, "a twin file in a soft handle"
        assert twin._lib.ga3c_ddpg_load(twin._h, path.encode()) == ESTATE, "a soft file in a twin handle"
        assert other._lib.ga3c_ddpg_load(other._h, path.encode()) == ESTATE, "another soft_config"
        assert _same(before_f, _snapshot(fresh)) and fresh.get_global_step() == 3
        assert _same(before_t, _snapshot(twin, t3.TRAINABLE)) and twin.get_global_step() == 1
        assert _same(before_o, _snapshot(other)) and other.get_global_step() == 0
    finally:
        for h in (fresh, twin, other):
            h.close()


def test_return_codes_and_destroy():
    import _native as nat
    from test_gpu_td3 import _tnet
    S, A, B = 3, 1, 16
    lib = nat.hip_lib()
    create, destroy = lib.ga3c_ddpg_soft_create, lib.ga3c_ddpg_soft_destroy
    good = (-1.6, 1.0, -1.0, -20.0, 2.0, 7)
    twin = _tnet(S, A, delay=2, max_batch=32, capacity=64)
    plain = _net(S, A, max_batch=32, capacity=64, DDPG_CRITIC_LOSS="paired")
    wide = _tnet(S, 17, delay=2, max_batch=32, capacity=64)
    busy = _tnet(S, A, delay=2, max_batch=32, capacity=64)
    try:
        h = twin._h
        nan, inf = float("nan"), float("inf")
        for bad in ((nan, 1.0, -1.0, -20.0, 2.0), (-1.6, nan, -1.0, -20.0, 2.0), (-1.6, 1.0, inf, -20.0, 2.0),
                    (-1.6, 1.0, -1.0, nan, 2.0), (-1.6, 1.0, -1.0, -20.0, inf), (-1.6, -0.5, -1.0, -20.0, 2.0),
                    (-1.6, 1.0, -1.0, 2.0, 2.0), (-1.6, 1.0, -1.0, 3.0, 2.0), (inf, 1.0, -1.0, -20.0, 2.0)):
            assert create(h, *bad, 7) == EINVAL, bad
        assert create(wide._h, *good) == EINVAL, "2A > 32"
        assert create(plain._h, *good) == ESTATE, "no twin critics"
        busy.actors_create(8, seed=5, updates=1, batch=16, draw_seed=1)
        assert create(busy._h, *good) == ESTATE, "device actors first"
        busy.actors_destroy()
        busy.eval_create(4, seed=1)
        assert create(busy._h, *good) == ESTATE, "evaluation episodes first"
        busy.eval_destroy()
        assert destroy(h) == ESTATE and lib.ga3c_ddpg_soft_info(h, None, None, None, None) == ESTATE
        buf = np.zeros(B * 400 + 1, np.float32)
        b = sc.candidates(S, A, B, np.random.default_rng(0))
        twin.train(*_args(b), noise=False)
        for name in SOFT_FETCH:
            assert lib.ga3c_ddpg_fetch(h, name.encode(), nat.ptr(buf), B) == ESTATE, name
        assert lib.ga3c_ddpg_get_param(h, so.LOG_ALPHA.encode(), 0, nat.ptr(buf), 1) == EINVAL
        before = {(k, w): twin.get_variable_value(k, w) for k in t3.ALL_VARS for w in (0, 1, 2, 3, 4)}
        assert create(h, *good) == 0
        assert create(h, *good) == ESTATE, "a second create"
        assert lib.ga3c_ddpg_twin_destroy(h) == ESTATE
        names = twin.get_variables_names()
        assert names == [k + ":0" for k in so.ALL_VARS] and twin.get_target_names()[38] == "actor_soft_1/log_alpha:0"
        head = ("actor_output/W", "actor_output/b")
        for (k, w), v in before.items():
            if k not in head:
                assert np.array_equal(v, twin.get_variable_value(k, w)), (k, w)
        for k in head:
            for w in (0, 1, 2, 3, 4):
                assert not twin.get_variable_value(k, w).any() and twin.get_variable_value(k, w).shape == so.shapes(S, A)[k]
        assert twin.get_variable_value(so.LOG_ALPHA, 0)[0] == twin.get_variable_value(so.LOG_ALPHA, 1)[0] == np.float32(-1.6)
        assert not any(twin.get_variable_value(so.LOG_ALPHA, w).any() for w in (2, 3, 4)) and twin._param_info(so.LOG_ALPHA)[2]
        assert twin.soft_info()[:2] == (np.float32(-1.6), -1.0)
        twin.train(*_args(b), noise=False)                        # t = 2 at delay 2: a policy step
        for name, width in SOFT_FETCH.items():
            width = A if width == "A" else width
            assert lib.ga3c_ddpg_fetch(h, name.encode(), nat.ptr(buf), B * width) == 0, name
            assert lib.ga3c_ddpg_fetch(h, name.encode(), nat.ptr(buf), B * width + 1) == EINVAL, name
        assert lib.ga3c_ddpg_fetch(h, b"do", nat.ptr(buf), B * 2 * A) == 0 and lib.ga3c_ddpg_fetch(h, b"do", nat.ptr(buf), B * A) == EINVAL
        twin.actors_create(8, seed=5, updates=1, batch=16, draw_seed=1)
        assert lib.ga3c_ddpg_envnoise_create(h, 3, 0) == ESTATE
        assert destroy(h) == ESTATE, "the device actors step under the policy"
        twin.actors_destroy()
        before = {(k, w): twin.get_variable_value(k, w) for k in t3.ALL_VARS for w in (0, 1, 2, 3, 4) if k not in head}
        assert destroy(h) == 0
        assert twin.get_variables_names() == [k + ":0" for k in t3.ALL_VARS]
        for k in head:
            for w in (0, 1, 2, 3, 4):
                assert not twin.get_variable_value(k, w).any() and twin.get_variable_value(k, w).shape == t3.shapes(S, A)[k]
        assert all(np.array_equal(v, twin.get_variable_value(k, w)) for (k, w), v in before.items())
        assert lib.ga3c_ddpg_fetch(h, b"s_mu", nat.ptr(buf), B * A) == ESTATE and lib.ga3c_ddpg_fetch(h, b"do", nat.ptr(buf), B * A) == 0
        twin.train(*_args(b), noise=False)                        # the twin's step again
        assert create(h, *good) == 0                              # ... and ga3c_ddpg_destroy takes a soft handle down too
    finally:
        for n in (twin, plain, wide, busy):
            n.close()


# ---- 10. the same calls give the same bits, also from a fresh handle

def test_repeated_steps_are_bit_identical_and_train_replay_is_train():
    S, A, B = 7, 3, 33
    rng = np.random.Generator(np.random.PCG64(11))
    online, target = so.random_params(S, A, rng), so.random_params(S, A, rng)
    s, a, r, done, s2 = sc.candidates(S, A, 128, rng)
    slots = np.random.default_rng(3).choice(128, B, replace=False).astype(np.int32)
    snaps = []
    for how in ("replay", "train", "replay"):
        net = _snet(S, A, delay=2)
        try:
            _load(net, online, target)
            assert net.replay_add(s, a, r, done, s2) == (128, 128)
            for _ in range(4):
                if how == "replay":
                    net.train_replay(slots, stamp=128, noise=False)
                else:
                    net.train(s[slots], r[slots], a[slots], s2[slots], done[slots], noise=False)
            snaps.append((_snapshot(net), {k: net.fetch(k, B * (A if w == "A" else w)) for k, w in SOFT_FETCH.items()},
                          net.fetch("do", B * 2 * A), net.soft_info()))
        finally:
            net.close()
    for other in snaps[1:]:
        assert _same(snaps[0][0], other[0]) and _same(snaps[0][1], other[1]) and np.array_equal(snaps[0][2], other[2])
        assert snaps[0][3] == other[3]


# ---- 11. both regimes under the Server

def _server_config(monkeypatch, tmp_path, extra):
    import ga3c_amd  # noqa: F401
    from Config import Config
    monkeypatch.chdir(tmp_path)
    for k, v in (("GAME", "Pendulum-v0"), ("USE_DDPG", True), ("DDPG_TWIN", True), ("DDPG_SOFT", True), ("DDPG_CRITIC_LOSS", "paired"),
                 ("DYNAMIC_SETTINGS", False), ("SAVE_MODELS", False), ("TRAINING_MIN_BATCH_SIZE", 64),
                 ("CONTINUOUS_INPUT", Config.CONTINUOUS_INPUT), ("DISCRATE_INPUT", Config.DISCRATE_INPUT),
                 ("DISCOUNTING", Config.DISCOUNTING), ("USE_REPLAY_MEMORY", Config.USE_REPLAY_MEMORY)) + extra:
        monkeypatch.setattr(Config, k, v)


def _served(srv, tmp_path):
    import os
    model = srv.model
    assert srv.failure is None and srv.training_step > 4 and model.get_global_step() == srv.training_step
    la, ent, mean_logp, predictions = model.soft_info()
    assert ent == -1.0 and predictions > 0 and np.isfinite([la, mean_logp]).all()
    assert la != float(np.float32(np.log(0.2))), "the temperature trained"
    for k in ("actor_output/W", "critic2_fc1/W", so.LOG_ALPHA):
        assert np.all(np.isfinite(model.get_variable_value(k, 0)))
    assert model.get_variable_value("actor_output/W", 0).shape == (300, 2)
    model.log(training_step=srv.training_step)
    soft = np.loadtxt(os.path.join("logs", model.model_name, "soft.csv"), delimiter=",", ndmin=2)
    assert soft.shape == (1, 3) and np.isclose(soft[0, 1], np.exp(la), rtol=1e-6)
    scalars = np.loadtxt(os.path.join("logs", model.model_name, "scalars.csv"), delimiter=",", ndmin=2)
    assert scalars.shape == (1, 4), "scalars.csv keeps its columns"


@pytest.mark.timeout(120)
def test_server_trains_pendulum_on_the_host_path(tmp_path, monkeypatch):
    _server_config(monkeypatch, tmp_path, (("AGENTS", 4), ("PREDICTORS", 1), ("TRAINERS", 1), ("TIME_MAX", 5),
                                           ("REPLAY_BUFFER_SIZE", 2000)))
    from Server import Server
    import NetworkDDPG
    srv = Server(max_agents=8)
    try:
        assert isinstance(srv.model, NetworkDDPG.Network) and srv.model.soft and len(srv.model.get_variables_names()) == 39
        srv.main(max_seconds=3)
        assert srv.predictions_served > 50
        _served(srv, tmp_path)
    finally:
        srv.model.close()


@pytest.mark.timeout(120)
def test_server_runs_the_device_actors_with_priorities_nstep_task_and_evaluation(tmp_path, monkeypatch):
    _server_config(monkeypatch, tmp_path, (("DEVICE_AGENTS", 64), ("DEVICE_DDPG", True), ("PRIORITIZED_REPLAY", True),
                                           ("REPLAY_BUFFER_SIZE", 65536), ("DDPG_NSTEP", 3), ("DEVICE_DDPG_ACTION_BOUND", "clip"),
                                           ("DEVICE_DDPG_TIME_LIMIT", "truncate"), ("DEVICE_DDPG_EVAL_ENVS", 16),
                                           ("DEVICE_DDPG_EVAL_EVERY", 50)))
    from Server import Server
    srv = Server()
    try:
        assert srv.model.soft and srv.model.prioritized and srv.model.nstep == 3 and srv.model.task is not None
        srv.main(max_seconds=3)
        _served(srv, tmp_path)
        assert open("results.txt").read().strip() or srv.training_step > 0
        import os
        ev = np.loadtxt(os.path.join("logs", srv.model.model_name, "eval.csv"), delimiter=",", ndmin=2)
        assert ev.shape[0] >= 1 and ev.shape[1] == 7 and np.all(np.isfinite(ev))
    finally:
        srv.model.close()
