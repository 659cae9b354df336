"""-m gpu: the DDPG handle from 448 to 4096 rows, the limit ga3c_ddpg_create admits -- on both sides of the two thread counts
past which a loop of csrc/ga3c_ddpg.hip takes a second trip (THREADS = 448: the sums over y of critic_step and ddpg_popart_kernel;
PER_THREADS = 1024: the draws and the weight maximum of per_sample_kernel, the rows of per_update_kernel) and at MAX_B = 4096,
where wgrad_element's serial float32 sums are the longest chains of the project.  tests/ddpg_batch_cases.py builds the cases,
tests/test_ddpg_batch_cpu.py asserts without a GPU what makes them worth running, tests/README.md ("The DDPG step past one pass
of its workgroups") has the reasons and what was observed.

Tolerances are the older files': _check (1e-4 x max(1, max|want|)) on rows and gradients, WTOL on weights and slots after steps,
PTOL on weights and priorities, bits on slots, draws and what the older files hold to bits; closeness.py (max(16 x e32, 2^-20)
per tensor) on every delta and gradient, e32 from the float32 oracle on the same rows or, where the cases say so, from the
restatement of the kernel's serial order.  One handle per (shape, option) with max_batch = 4096 serves all its sizes: a test
loads both nets, both optimizer slots and the step counter before it runs.  (A handle with priorities counts its draws, and the
oracle's draw is that of a sample number: those handles serve one test each.)"""
import numpy as np
import pytest

import closeness as cl
import ddpg_actors_oracle as do
import ddpg_batch_cases as bc
import ddpg_oracle as o
import per_oracle as per
from test_gpu_ddpg import LR, WTOL, _check, _compare_step4, _load, _net, _same, _snapshot

pytestmark = pytest.mark.gpu

_HANDLES = {}


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    while _HANDLES:
        _HANDLES.popitem()[1].close()


def _handle(key, make):
    if key not in _HANDLES:
        _HANDLES[key] = make()
    return _HANDLES[key]


def _reset(net, st, names=o.TRAINABLE, load=_load, lr=LR):
    """Both nets, both optimizer slots and the step counter as the oracle's fresh state `st` has them."""
    load(net, st["online"], st["target"])
    for k in names:
        net.set_variable_value(k, st["slot_a"][k], 2)
        net.set_variable_value(k, st["slot_b"][k], 3)
    net.set_global_step(0)
    net.learning_rate = lr
    assert net.get_global_step() == 0


def _args(b):
    return b[0], b[2], b[1], b[4], b[3]          # Network.train's order: x, y_r, a, x2, done


def _relative(label, items, failed):
    """items: (name, got, want, e32) through closeness.py -> the worst rel_err / bound; misses are appended to `failed`."""
    worst = (0.0, None)
    for name, got, want, e32 in items:
        bound = cl.bound(e32)
        err = cl.report(label, name, got, want, e32, bound)
        worst = max(worst, (err / bound, name))
        if not err <= bound:
            failed.append((name, err, bound))
    print("WORST %s: rel_err / bound %.3f (%s)" % ((label,) + worst))
    return worst


# ---- 1. the plain handle, steps 1 - 4

ROW_PARAMS = [(S, A, B, form) for S, A, B in bc.ROW_CASES for form in bc.FORMS]


@pytest.mark.parametrize("S,A,B,form", ROW_PARAMS, ids=["S%d-A%d-B%d-%s" % p for p in ROW_PARAMS])
def test_every_row_and_gradient(S, A, B, form):
    """y, qt, q, dq, q_max, q_avg, every kept activation and delta and every gradient of both nets by _check, then every delta
    and gradient by closeness.py.  In the fork form every row's dq carries the mean of y over ALL rows (critic_step's strided
    sum); every gradient element is a serial sum over all rows."""
    case = bc.row_case(S, A, B, form)
    net = _handle(("plain", S, A, form), lambda: _net(S, A, max_batch=bc.MAX_B, capacity=bc.CAPACITY, DDPG_CRITIC_LOSS=form))
    _reset(net, o.new_state(case.online, case.target), lr=bc.ROWS_LR)
    q_max, q_avg = net.compute(*_args(case.batch), 4, noise=case.noise)
    _check("q_max", [q_max], [case.out["q_max"]])
    _check("q_avg", [q_avg], [case.out["q_avg"]])
    _compare_step4(net, case.out, S, A, B)
    for k in o.CRITIC_TRAINABLE:
        _check("after step 3 " + k, net.get_variable_value(k, 0), case.st["online"][k], WTOL)
    assert net.get_global_step() == 0
    for k, (blas, serial) in case.restated.items():
        print("e32 restated S=%d A=%d B=%d %s %s: BLAS %.3e serial %.3e" % (S, A, B, form, k, blas, serial))
    failed, items = [], []
    for name, want in case.want.items():
        got = net.get_variable_value(name[5:], 4) if name.startswith("grad ") else net.fetch(name, np.size(want))
        items.append((name, got, want, case.e32[name]))
    _relative("ddpg S=%d A=%d B=%d %s" % (S, A, B, form), items, failed)
    assert not failed, failed


# ---- 2. two full steps

@pytest.mark.parametrize("B", bc.STEP_SIZES)
@pytest.mark.parametrize("way", list(bc.STEP_WAYS))
def test_two_full_steps_and_train_replay_on_the_same_rows(way, B):
    """Online weights, targets, both optimizer slots and the step counter after two steps of train() (test_gpu_ddpg's
    test_two_full_steps at LR with critic_lr = 1), then the same two steps as train_replay on ring slots: the same bits."""
    S, A = bc.SHAPE
    case = bc.step_case(B, way)
    net = _handle(("steps", way), lambda: _net(S, A, max_batch=bc.MAX_B, capacity=bc.CAPACITY, critic_lr=bc.STEPS_CRITIC_LR, **case.cfg))
    fresh = o.new_state(case.online, case.target, critic_rmsprop=case.cfg.get("RMSPROP", True))
    _reset(net, fresh)
    for i, (b, out) in enumerate(zip(case.batches, case.outs)):
        q_max, q_avg = net.train(*_args(b), noise=case.noise)
        _check("step %d q_max" % i, [q_max], [out["q_max"]])
        _check("step %d q_avg" % i, [q_avg], [out["q_avg"]])
        if i == 0:
            for k in o.TRAINABLE:          # targets after step 0: the one-soft-update rule on the loaded targets
                _check("target rule " + k, net.get_variable_value(k, 1), 0.001 * case.after_first[k] + 0.999 * case.target[k], WTOL)
    assert net.get_global_step() == 2
    st = case.st
    for k in o.TRAINABLE:
        _check("online " + k, net.get_variable_value(k, 0), st["online"][k], WTOL)
        _check("target " + k, net.get_variable_value(k, 1), st["target"][k], WTOL)
        _check("slot a " + k, net.get_variable_value(k, 2), st["slot_a"][k], WTOL)
        _check("slot b " + k, net.get_variable_value(k, 3), st["slot_b"][k], WTOL)
    assert np.array_equal(net.get_variable_value(o.DEAD, 0), case.online[o.DEAD].astype(np.float32)), "critic_fc2/b moved"
    trained = _snapshot(net)
    _reset(net, fresh)
    for b in case.batches:
        size, total = net.replay_add(*b)
        slots = ((total - B + np.arange(B)) % bc.CAPACITY).astype(np.int32)
        net.train_replay(slots, stamp=total, noise=case.noise)
    assert net.get_global_step() == 2
    assert _same(trained, _snapshot(net)), "train_replay differs from train on the same rows"


# ---- 3. prioritised replay

def _per_ring(kind, **kw):
    """-> (a fresh handle on the ring `kind` of the cases, full, with the cases' priorities; size, pa, max_pa).  Fresh, because a
    handle's sample counter runs on: the cases' sample numbers are those of a handle that has drawn nothing else."""
    from test_gpu_prioritized_replay import _add, _per_net, _rows
    capacity, pa, top = bc.ring(kind)
    net = _per_net(capacity, max_batch=bc.MAX_B, **kw)
    try:
        if kind == "million":
            zeros = tuple(np.zeros((bc.MAX_B,) + t.shape[1:], np.float32) for t in _rows(1, np.random.default_rng(0)))
            for _ in range(capacity // bc.MAX_B):
                got = net.replay_add(*zeros)
            assert got == (capacity, capacity)
        else:
            assert _add(net, _rows(capacity, np.random.default_rng(capacity))) == (capacity, capacity)
        net.set_priorities(pa, top)
    except BaseException:
        net.close()
        raise
    return net, capacity, pa, top


@pytest.mark.parametrize("kind", list(bc.DRAWS))
def test_draw_equals_the_oracle_slot_for_slot(kind):
    """per_sample_kernel past one pass of its 1024 threads: the slots equal per_oracle.draw's, the weights are within PTOL and
    their largest is exactly 1 (the maximum folds every row a thread drew: on the 'tail' ring only row 1024 of 1025, the second
    row of thread 0, reaches it), on a ring a little larger than the batch, on the largest ring and on the heavy-tailed one."""
    from test_gpu_prioritized_replay import PTOL, _rel
    net, size, pa, top = _per_ring(kind)
    try:
        got_pa, got_top = net.priorities()
        assert np.array_equal(got_pa, pa) and got_top == np.float32(top)
        net.replay_beta = 0.4
        assert [n for _, n in bc.DRAWS[kind]] == list(range(len(bc.DRAWS[kind])))
        for B, number in bc.DRAWS[kind]:
            slots, w = net.sample_prioritized(B)
            want, total, clamped = bc.draw(kind, B, number)
            print("ring %s B %d: clamped %d, duplicates %d, slot %d in %d rows" % (kind, B, clamped, B - len(set(want.tolist())),
                                                                                  bc.HEAVY_SLOT, int((want == bc.HEAVY_SLOT).sum())))
            assert slots.dtype == np.int32 and np.array_equal(slots, want), (B, np.flatnonzero(slots != want)[:8])
            err = _rel(w, per.weights(pa, size, want, total, 0.4))
            print("ring %s B %d: weights within %.2e" % (kind, B, err))
            assert err <= PTOL and w.max() == 1.0
            assert np.array_equal(net.fetch("per_w", B), w)
        again, top2 = net.priorities()
        assert np.array_equal(again, pa) and top2 == got_top and net.get_global_step() == 0
    finally:
        net.close()


@pytest.mark.parametrize("kind,B", bc.UPDATES)
def test_update_on_the_heavy_tailed_draw(kind, B):
    """per_update_kernel with sl[] filled past 1024 entries and a slot named by hundreds of rows: pa, max_pa and td against
    per_oracle.update on the fetched y and q, as test_update_with_duplicates_keeps_the_last_row... compares them.  (4096 rows
    are drawn from the same priorities on 4100 slots: train_prioritized wants more rows than a batch.)"""
    from test_gpu_prioritized_replay import ALPHA, EPS, PTOL, _check_update, _rel
    net, size, pa, top = _per_ring(kind)
    try:
        rng = np.random.Generator(np.random.PCG64(81))
        S, A = bc.PER_SHAPE
        online, target = o.random_params(S, A, rng), o.random_params(S, A, rng)
        _load(net, online, target)
        net.replay_beta = 0.4
        net.train_prioritized(B, noise=False)
        slots = net.last_slots
        assert np.array_equal(slots, bc.draw(kind, B, 0)[0])
        named = np.flatnonzero(slots == bc.HEAVY_SLOT)
        assert named.size > 0.9 * B
        after, new_top = _check_update(net, pa, np.float32(top), slots, B)
        y, q = net.fetch("y", B), net.fetch("q", B)
        want = pa.copy()
        want_top = per.update(want, top, slots, y, q, EPS, ALPHA)
        assert _rel(after, want) <= PTOL and abs(float(new_top) - float(want_top)) <= PTOL * float(want_top)
        assert new_top == np.float32(top)             # 50 was the largest before and stays it
        _, p = per.new_priorities(y, q, EPS, ALPHA)
        assert abs(float(after[bc.HEAVY_SLOT]) - p[named[-1]]) <= PTOL * p[named[-1]], "the slot most rows name holds the last row's"
        assert net.get_global_step() == 1
    finally:
        net.close()


def test_weighted_step_at_1025_rows():
    """One weighted step (beta 0.4) against per_oracle.train_step, as test_weighted_step_matches_the_oracle holds it, at LR with
    critic_lr = 1: a thread of per_sample_kernel draws two rows and the weights reach dq of every row."""
    from test_gpu_prioritized_replay import PTOL, _add, _check_update, _f64, _per_net, _rel
    pa, want_slots, want_w, noise, online, target, rows = bc.weighted_case()
    n, B, beta = bc.WEIGHTED["n"], bc.WEIGHTED["B"], bc.WEIGHTED["beta"]
    net = _per_net(n, max_batch=bc.MAX_B, critic_lr=bc.STEPS_CRITIC_LR)
    try:
        _load(net, online, target)
        assert _add(net, rows) == (n, n)
        net.set_priorities(pa, 0.05)
        net.replay_beta = beta
        q_max, q_avg = net.train_prioritized(B, noise=noise)
        slots, w = net.last_slots, net.fetch("per_w", B)
        assert np.array_equal(slots, want_slots) and _rel(w, want_w) <= PTOL
        assert len(np.unique(w)) > B // 2, "the weights do not vary"
        st = o.new_state(online, target)
        batch = _f64(tuple(t[slots] for t in rows))
        out = per.train_step(st, *batch, w.astype(np.float64), LR, noise.astype(np.float64), critic_lr=bc.STEPS_CRITIC_LR)
        t4 = o.critic_forward(st["online"], batch[0], out["a_out"])["t"]
        assert np.abs(t4).min() > 9e-5, "the fetched weights moved a row of the batch onto a relu's edge"
        _check("q_max", [q_max], [out["q"].max()])
        _check("q_avg", [q_avg], [out["q"].mean()])
        for name in ("y", "q", "dq"):
            _check(name, net.fetch(name, B), out[name])
        unweighted = (2.0 / B) * (out["q"] - out["y"])
        assert np.max(np.abs(out["dq"] - unweighted)) > 0.1 * np.max(np.abs(out["dq"])), "the weights did not reach the oracle's loss"
        for k in o.CRITIC_TRAINABLE:
            _check("grad " + k, net.get_variable_value(k, 4), out["critic_grads"][k])
        for k in o.ACTOR_TRAINABLE:
            _check("grad " + k, net.get_variable_value(k, 4), out["actor_grads"][k])
        for k in o.TRAINABLE:
            _check("online " + k, net.get_variable_value(k, 0), st["online"][k], WTOL)
            _check("target " + k, net.get_variable_value(k, 1), st["target"][k], WTOL)
            _check("slot a " + k, net.get_variable_value(k, 2), st["slot_a"][k], WTOL)
            _check("slot b " + k, net.get_variable_value(k, 3), st["slot_b"][k], WTOL)
        assert net.get_global_step() == 1
        _check_update(net, pa, np.float32(0.05), slots, B)
    finally:
        net.close()


# ---- 4. PopArt

@pytest.mark.parametrize("B", bc.OPTION_SIZES)
def test_popart_statistics_rescale_and_step(B):
    """ddpg_popart_kernel's strided f64 sums and yn loop past 448 rows, from statistics near -100 at beta = 0.5.  With lr = 0, as
    test_the_kernel_alone: mu', nu' within one f32 spacing of popart_oracle.update_mixed (its sums are kernel_sums, the kernel's
    order), and from the stored statistics on the oracle's expressions give the kernel's bits -- the rescaled head of both nets,
    yn of every row, sigma'.  Then the step at ROWS_LR: rows and gradients against popart_oracle.train_step."""
    import popart_oracle as po
    from test_gpu_popart import MU, NU, _compare_rows, _set_stats, _stats
    from test_gpu_ddpg_actors import _eq
    S, A = bc.SHAPE
    online, target, batch, noise, kw = bc.popart_case(B)
    s, a, r, done, s2 = batch
    net = _handle(("popart",), lambda: _net(S, A, max_batch=bc.MAX_B, capacity=bc.CAPACITY, DDPG_POPART=True,
                                            DDPG_POPART_BETA=bc.POPART_BETA, DDPG_CRITIC_LOSS="paired",
                                            DDPG_FUTURE_REWARD_CALC=False))
    mu, nu = np.float32(bc.POPART_MU), np.float32(bc.POPART_NU)
    # the kernel alone
    _reset(net, o.new_state(online, target), lr=0.0)
    _set_stats(net, mu, nu)
    net.compute(s, r, a, s2, done, 3, noise=False)
    y = net.fetch("y", B)
    assert _eq(y, r)
    mu1, nu1 = (np.float32(v) for v in _stats(net))
    want_mu, want_nu = po.update_mixed(mu, nu, y, bc.POPART_BETA)
    s1, s2sum = po.kernel_sums(y)
    print("B %d: sums %.17g %.17g  mu' %.9g (oracle %.9g)  nu' %.9g (oracle %.9g)" % (B, s1, s2sum, mu1, want_mu, nu1, want_nu))
    assert abs(float(mu1) - float(want_mu)) <= np.spacing(np.abs(want_mu))
    assert abs(float(nu1) - float(want_nu)) <= np.spacing(np.abs(want_nu))
    assert _eq(net.get_variable_value(MU, 1)[0], mu1) and _eq(net.get_variable_value(NU, 1)[0], nu1)
    ratio, shift, muf, isig, sigma, sigma1 = po.constants(mu, nu, mu1, nu1)
    for which, P in ((0, online), (1, target)):
        W, b = po.rescale(P[po.WO].astype(np.float32), P[po.BO].astype(np.float32), ratio, shift)
        assert _eq(net.get_variable_value(po.WO, which), W), which
        assert _eq(net.get_variable_value(po.BO, which), b), which
    assert _eq(net.fetch("yn", B), po.normalise(y, muf, isig))
    info = net.popart_info()
    assert info[1:3] == (float(mu1), float(nu1)) and info[3] == float(np.float32(sigma1))
    assert po.bounds32()[0] < sigma1 < po.bounds32()[1]
    # the step
    st = po.new_state(online, target, mu=float(mu), nu=float(nu))
    _reset(net, st, lr=bc.ROWS_LR)
    _set_stats(net, mu, nu)
    out = po.train_step(st, *bc.f64(batch), bc.ROWS_LR, noise.astype(np.float64), stop_after=4, mixed=False, **kw)
    q_max, q_avg = net.compute(s, r, a, s2, done, 4, noise=noise)
    _check("q_max", [q_max], [out["q_max"]])             # return units
    _check("q_avg", [q_avg], [out["q_avg"]])
    _compare_rows(net, out, B, names=("y", "yn", "q", "dq"))
    fc, fa = out["critic_fwd"], out["actor_fwd"]
    for name, want in (("c_dt", fc["dt"]), ("c_dn1", fc["dn1"]), ("g", out["g"]), ("do", fa["do"]), ("a_dn2", fa["dn2"]), ("a_dn1", fa["dn1"])):
        _check(name, net.fetch(name, np.size(want)), want)
    for k in o.CRITIC_TRAINABLE:
        _check("grad " + k, net.get_variable_value(k, 4), out["critic_grads"][k])
    for k in o.ACTOR_TRAINABLE:
        _check("grad " + k, net.get_variable_value(k, 4), out["actor_grads"][k])
    got_mu, got_nu = _stats(net)
    _check("mu", [got_mu], [st["mu"]], WTOL)
    _check("nu", [got_nu], [st["nu"]], WTOL)
    # the tensors the normalised targets reach, relative to their own largest entry: e32 from the oracle's mixed float32 run
    s32 = po.new_state(bc.f32(online), bc.f32(target), mu=float(mu), nu=float(nu))
    w32 = po.train_step(s32, *batch, np.float32(bc.ROWS_LR), noise, stop_after=4, mixed=True, **kw)
    failed, items = [], []
    for k in o.CRITIC_TRAINABLE:
        if k != o.DEAD:
            assert w32["critic_grads"][k].dtype == np.float32
            e32 = cl.rel_err(w32["critic_grads"][k], out["critic_grads"][k])
            if k == "critic_output/b":
                e32 = max(e32, cl.e32_of_row_sum(w32["dq"], out["dq"]))
            items.append(("grad " + k, net.get_variable_value(k, 4), out["critic_grads"][k], e32))
    _relative("popart B=%d" % B, items, failed)
    assert not failed, failed


# ---- 5. twin, distributional, soft

@pytest.mark.parametrize("B", bc.OPTION_SIZES)
def test_twin_step_every_row_and_both_critics(B):
    """test_gpu_td3._every_row at ROWS_LR with sigma = 1, c = 0.3 (the clip applies to most draws): 256 tiles x 2 critics in one
    grid, and the smoothing draws j = row A + i up to 4096 x 3, held to td3_oracle.smoothing_noise bit for bit."""
    import td3_oracle as t3
    from test_gpu_td3 import _load as load, _single_draws, _tnet
    S, A = bc.SHAPE
    online, target, batch, noise, _ = bc.twin_case(B)
    tw = bc.TWIN
    net = _handle(("twin",), lambda: _tnet(S, A, delay=1, sigma=tw["sigma"], c=tw["noise_clip"], max_batch=bc.MAX_B, capacity=bc.CAPACITY))
    _reset(net, t3.new_state(online, target), names=t3.TRAINABLE, load=load, lr=bc.ROWS_LR)
    q_max, q_avg = net.compute(*_args(batch), 4, noise=noise)
    eps = net.fetch("t_eps", B * A).reshape(B, A)
    want_eps = t3.smoothing_noise(bc.TWIN_SEED, 1, B, A, tw["sigma"], tw["noise_clip"])
    differ = np.flatnonzero(eps.view(np.uint32).ravel() != want_eps.view(np.uint32).ravel())
    print("t_eps: %d of %d draws differ in bits, max |device - numpy| %.3e, %d at the clip"
          % (differ.size, eps.size, float(np.max(np.abs(eps.astype(np.float64) - want_eps))),
             int((np.abs(want_eps) == np.float32(tw["noise_clip"])).sum())))
    assert differ.size == 0, differ[:8]
    st = t3.new_state(online, target)
    out = t3.train_step(st, *bc.f64(batch), bc.ROWS_LR, noise.astype(np.float64), eps=eps, stop_after=4, **tw)
    w32 = t3.train_step(t3.new_state(bc.f32(online), bc.f32(target)), *batch, bc.ROWS_LR, noise, eps=eps, stop_after=4, **tw)
    _check("q_max", [q_max], [out["q_max"]])
    _check("q_avg", [q_avg], [out["q_avg"]])
    f1, f2, fa = out["critic_fwd"], out["critic2_fwd"], out["actor_fwd"]
    rows = [("y", out["y"]), ("qt", out["qt"]), ("qt1", out["qt1"]), ("qt2", out["qt2"]), ("t_a", out["t_a"]),
            ("q", out["q"]), ("dq", out["dq"]), ("c_xh1", f1["xh1"]), ("c_c1", f1["c1"]), ("c_c2", f1["c2"]), ("c_dt", f1["dt"]),
            ("c_dn1", f1["dn1"]), ("q2", out["q2"]), ("dq2", out["dq2"]), ("c2_xh1", f2["xh1"]), ("c2_c1", f2["c1"]),
            ("c2_c2", f2["c2"]), ("c2_dt", f2["dt"]), ("c2_dn1", f2["dn1"]),
            ("c2_dh1", f2["dn1"] * (online["critic2_norm1/gamma"] * f2["rs1"])),
            ("a_xh1", fa["xh1"]), ("a_a1", fa["a1"]), ("a_xh2", fa["xh2"]), ("a_a2", fa["a2"]), ("a_out", fa["out"]),
            ("a_noisy", out["a_out"]), ("g", out["g"]), ("do", fa["do"]), ("a_dn2", fa["dn2"]), ("a_dn1", fa["dn1"])]
    for name, want in rows:
        _check(name, net.fetch(name, np.size(want)), want)
    assert np.array_equal(net.fetch("qt", B), np.minimum(net.fetch("qt1", B), net.fetch("qt2", B)))
    failed, items = [], []
    draws = _single_draws(S, A, B, online, target, batch, eps, out, w32)
    for pre, tag in (("critic_", "critic_grads"), ("critic2_", "critic2_grads")):
        for k in o.CRITIC_TRAINABLE:
            name = pre + k[len("critic_"):]
            got = net.get_variable_value(name, 4)
            _check("grad " + name, got, out[tag][k])
            if k != o.DEAD:
                assert w32[tag][k].dtype == np.float32
                items.append(("grad " + name, got, out[tag][k], max(cl.rel_err(w32[tag][k], out[tag][k]), draws[tag][k] or 0.0)))
    for k in o.ACTOR_TRAINABLE:
        got = net.get_variable_value(k, 4)
        _check("grad " + k, got, out["actor_grads"][k])
        assert w32["actor_grads"][k].dtype == np.float32
        items.append(("grad " + k, got, out["actor_grads"][k], cl.rel_err(w32["actor_grads"][k], out["actor_grads"][k])))
    _relative("td3 B=%d" % B, items, failed)
    assert not failed, failed
    for k in o.CRITIC_TRAINABLE + t3.CRITIC2_TRAINABLE:
        _check("after step 3 " + k, net.get_variable_value(k, 0), st["online"][k], WTOL)
    assert net.get_global_step() == 0


@pytest.mark.parametrize("B", bc.OPTION_SIZES)
def test_distributional_step_every_row_and_gradient(B):
    """test_gpu_dist's test_every_row_and_gradient at ROWS_LR and 51 atoms: the projection's row stride of 51 out to row 4095."""
    import dist_oracle as d4
    from test_gpu_dist import _dnet, _kinds, _single_draws
    S, A = bc.SHAPE
    N, kw = bc.ATOMS, bc.DIST_KW
    online, target, batch, noise, _ = bc.dist_case(B)
    kinds = _kinds(batch, N)
    print("rows: %d done, %d clipped below, %d above, %d done on an atom" % tuple(int(k.sum()) for k in kinds))
    assert all(k.any() for k in kinds)
    net = _handle(("dist",), lambda: _dnet(S, A, N, max_batch=bc.MAX_B, capacity=bc.CAPACITY, vmin=bc.VMIN, vmax=bc.VMAX))
    assert net.dist_info() == (N, bc.VMIN, bc.VMAX)
    _reset(net, d4.new_state(online, target), lr=bc.ROWS_LR)
    q_max, q_avg = net.compute(*_args(batch), 4, noise=noise)
    st = d4.new_state(online, target)
    out = d4.train_step(st, *bc.f64(batch), bc.ROWS_LR, noise.astype(np.float64), stop_after=4, **kw)
    w32 = d4.train_step(d4.new_state(bc.f32(online), bc.f32(target)), *batch, bc.ROWS_LR, noise, stop_after=4, **kw)
    _check("q_max", [q_max], [out["q_max"]])
    _check("q_avg", [q_avg], [out["q_avg"]])
    fc, fa = out["critic_fwd"], out["actor_fwd"]
    rows = [("y", out["y"]), ("qt", out["qt"]), ("d_pt", out["pt"]), ("d_m", out["m"]), ("d_p", out["p"]), ("d_dz", out["dz"]),
            ("d_ce", out["ce"]), ("q", out["q"]), ("c_x", batch[0]), ("c_a", batch[1]), ("c_xh1", fc["xh1"]), ("c_c1", fc["c1"]),
            ("c_c2", fc["c2"]), ("c_dt", fc["dt"]), ("c_dn1", fc["dn1"]), ("c_dh1", fc["dh1"]),
            ("a_xh1", fa["xh1"]), ("a_a1", fa["a1"]), ("a_xh2", fa["xh2"]), ("a_a2", fa["a2"]), ("a_out", fa["out"]),
            ("a_noisy", out["a_out"]), ("g", out["g"]), ("do", fa["do"]), ("a_dn2", fa["dn2"]), ("a_dn1", fa["dn1"])]
    for name, want in rows:
        _check(name, net.fetch(name, np.size(want)), want)
    m = net.fetch("d_m", B * N).reshape(B, N)
    assert np.max(np.abs(m.astype(np.float64).sum(axis=1) - 1.0)) <= 1e-5 and np.all(m >= 0.0)
    failed, items = [], []
    draws = _single_draws(S, A, B, N, online, target, out, w32, kw)
    for k in o.CRITIC_TRAINABLE:
        got = net.get_variable_value(k, 4)
        _check("grad " + k, got, out["critic_grads"][k])
        if k != o.DEAD:
            assert w32["critic_grads"][k].dtype == np.float32
            items.append(("grad " + k, got, out["critic_grads"][k],
                          max(cl.rel_err(w32["critic_grads"][k], out["critic_grads"][k]), draws[k] or 0.0)))
    for k in o.ACTOR_TRAINABLE:
        got = net.get_variable_value(k, 4)
        _check("grad " + k, got, out["actor_grads"][k])
        items.append(("grad " + k, got, out["actor_grads"][k], cl.rel_err(w32["actor_grads"][k], out["actor_grads"][k])))
    _relative("dist B=%d" % B, items, failed)
    assert not failed, failed
    for k in o.CRITIC_TRAINABLE:
        _check("after step 3 " + k, net.get_variable_value(k, 0), st["online"][k], WTOL)
    assert net.get_global_step() == 0


@pytest.mark.parametrize("B", bc.OPTION_SIZES)
def test_soft_policy_step_every_row_and_gradient(B):
    """test_gpu_sac's test_one_policy_step_every_row_and_gradient (its _policy_step, its cases' rule and seeds) at (7, 3): the
    [B, 2A] head, the draws of both streams out to row 4095, and the serial sum of logp behind the temperature's gradient."""
    import sac_oracle as so
    from test_gpu_sac import _load as load, _policy_step, _snet
    S, A = bc.SHAPE
    online, target, batch, _ = bc.soft_case(B)
    net = _handle(("soft",), lambda: _snet(S, A, delay=1, max_batch=bc.MAX_B, capacity=bc.CAPACITY))
    _reset(net, so.new_state(online, target), names=so.TRAINABLE, load=load, lr=bc.ROWS_LR)
    _policy_step(net, online, target, batch, bc.ROWS_LR, S, A, B)


# ---- 6. the uniform draw of the device actors

def test_the_device_actors_uniform_draw_at_1025_and_4096_rows():
    """ddpg_uniform_slots_kernel past one block of 256 threads: one actor step whose train step draws `batch` rows from a ring
    that holds more.  The slots are ddpg_actors_oracle.uniform_slots' and distinct."""
    from test_gpu_ddpg_actors import _weights
    from test_gpu_prioritized_replay import _add, _rows
    S, A = do.S, do.A
    net = _net(S, A, max_batch=bc.MAX_B, capacity=bc.CAPACITY)
    try:
        _load(net, *_weights(31))
        assert _add(net, _rows(bc.ACTORS_PREFILL, np.random.default_rng(6))) == (bc.ACTORS_PREFILL, bc.ACTORS_PREFILL)
        net.actors_create(bc.ACTORS_N, seed=5, updates=1, batch=bc.ACTORS_SIZES[0], draw_seed=bc.DRAW_SEED)
        for number, B in enumerate(bc.ACTORS_SIZES):
            net.actors_set("batch", B)
            assert net.actors_get("batch") == B and net.actors_get("draw_seed") == bc.DRAW_SEED
            stats = net.actors_run(1, train=True, noise=[0.3])
            size = net.replay_size()[0]
            print("actors B %d: stats %s, ring %d" % (B, stats, size))
            assert stats[:3] == (bc.ACTORS_N, 1, B) and size > B
            slots = net.actors_get("slots")
            assert slots.shape == (B,) and np.array_equal(slots, do.uniform_slots(bc.DRAW_SEED, number, size, B))
            assert len(set(slots.tolist())) == B and slots.min() >= 0 and slots.max() < size
        assert net.get_global_step() == len(bc.ACTORS_SIZES)
    finally:
        net.close()
