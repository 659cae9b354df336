"""The conditions tests/test_gpu_ddpg_saturation.py relies on, asserted on the oracle alone (tests/ddpg_saturation_cases.py builds
the cases of both files), and the proof that its element-wise check of 1 - tanh^2 is not vacuous: the KNOWN-WRONG float32 form
1 - o * o fails it and the engine's form, restated in numpy float32, passes it (the pattern of test_closeness_cpu.py).  Nothing
here touches a kernel or a GPU.

Why the oracle changed with these tests: ddpg_oracle.actor_grads used 1 - out^2, which at |h| > 19 is wrong by 100 % in float64
too, and in float32 (the run that supplies e32) from |h| = 9 on.  It now takes the derivative from the pre-activation."""
import numpy as np
import pytest

import closeness as cl
import ddpg_oracle as o
import ddpg_saturation_cases as sc


# ---- 0. the oracle's own statement of 1 - tanh^2

def test_dtanh_keeps_its_relative_accuracy_and_its_dtype():
    h = np.linspace(-45.0, 45.0, 1801)
    want = sc.dtanh_exact(h)
    assert np.max(np.abs(o.dtanh(h) / want - 1.0)) <= 2.0 ** -48
    h32 = h.astype(np.float32)
    got = o.dtanh(h32)
    assert got.dtype == np.float32 and np.all(got > 0)
    # float32, where the result is a normal number: exp's argument -2 |h| is exact, and a handful of roundings follow
    normal = sc.dtanh_exact(h32) >= sc.NORMAL
    assert normal.sum() > 1600 and np.max(np.abs(got[normal].astype(np.float64) / sc.dtanh_exact(h32[normal]) - 1.0)) <= 8 * 2.0 ** -24
    # the form it replaces, at the same points
    old = 1.0 - np.tanh(h) ** 2
    assert np.max(np.abs(old / want - 1.0)) >= 1.0 and not old[np.abs(h) > 20].any()


def test_the_oracle_stays_dtype_faithful():
    c = sc.actor(3, 1, 2)
    fa = c.w32["actor_fwd"]
    for k in ("ho", "out", "do", "dn2", "dn1"):
        assert fa[k].dtype == np.float32, k
    assert all(g.dtype == np.float32 for g in c.w32["actor_grads"].values())
    assert c.out["actor_fwd"]["ho"].dtype == np.float64
    assert np.array_equal(c.out["actor_fwd"]["out"], np.tanh(c.out["actor_fwd"]["ho"]))


def test_at_unsaturated_weights_the_delta_moves_by_rounding_only():
    """With weights as drawn (no scale) the new form moves `do` by rounding alone, in the float32 run too: 1 - out^2 carries
    an ABSOLUTE error of about 4 u (out and its square rounded, values near 1), dtanh a relative one of as much on a value that
    is at most 1; u = eps / 2.  So the bounds of the tests that were there before are measured on the same numbers."""
    for S, A in ((3, 1), (7, 3)):
        c = sc.actor(S, A)
        for run in (c.out, c.w32):
            fa = run["actor_fwd"]
            g = np.asarray(run["g"], fa["out"].dtype)
            old = -g * (1.0 - fa["out"] ** 2)
            moved = float(np.max(np.abs(old.astype(np.float64) - fa["do"])))
            print("S=%d A=%d %s: do moved by %.2e of its largest entry" % (S, A, g.dtype, moved / np.max(np.abs(fa["do"]))))
            assert moved <= 4 * np.finfo(g.dtype).eps * float(np.max(np.abs(g))), (S, A, g.dtype)


# ---- 1. the saturated actor

@pytest.mark.parametrize("S,A,k", sc.ACTOR_CASES)
def test_saturated_actor_conditions_and_the_two_forms(S, A, k):
    c = sc.actor(S, A, k)
    fa, f32 = c.out["actor_fwd"], c.w32["actor_fwd"]
    ho, ho32 = fa["ho"], f32["ho"]
    assert c.batch[0].shape == (sc.B, S) and ho.shape == (sc.B, A) and ho32.dtype == np.float32
    assert np.all(np.abs(c.noise) >= 0.05)
    share = float(np.mean(np.abs(ho) > sc.SATURATED))
    want = sc.dtanh_exact(ho)
    print("S=%d A=%d k=%d: max|h| %.1f, %.0f %% of the units beyond %.0f, smallest 1 - tanh^2 2^%.0f"
          % (S, A, k, np.abs(ho).max(), 100 * share, sc.SATURATED, np.log2(want.min())))
    assert share >= 0.10
    assert want.min() >= sc.NORMAL
    assert np.min(np.abs(np.abs(c.out["a_out"]) - 1.0)) > 1e-4, "a noisy action at the wrap's jump"
    assert np.all(c.out["g"] != 0), "the element-wise check would skip a unit"
    # the element-wise criterion of the GPU test on two numpy restatements in float32, both from the float32 oracle's h
    dh, bound = sc.dtanh_bound(ho32, ho)
    one, two, four = np.float32(1), np.float32(2), np.float32(4)
    out32 = np.tanh(ho32)
    wrong = one - out32 * out32
    e = np.exp(-two * np.abs(ho32))
    right = four * e / ((one + e) * (one + e))
    assert wrong.dtype == right.dtype == np.float32
    err_wrong, err_right = sc.dtanh_err(wrong, ho), sc.dtanh_err(right, ho)
    print("    dh %.3e bound %.3e: 1 - o o %.3e, 4 e / (1 + e)^2 %.3e" % (dh, bound, err_wrong, err_right))
    assert err_right <= bound
    assert err_wrong > bound and err_wrong >= 1.0          # a unit off by 100 %, not a near miss
    # ... and carried through the delta, as the GPU test reads it: r = -do / g
    g32 = np.asarray(c.w32["g"], np.float32)
    for form, passes in ((right, True), (wrong, False)):
        do = (-g32 * form).astype(np.float32)
        assert (sc.dtanh_err(-do.astype(np.float64) / g32, ho) <= bound) == passes
    # what 1e-4 x max(1, max|want|) sees of the wrong form: nothing.  (The tensor-relative comparator sees it only where every
    # unit of the batch is far out, so that the largest entry of `do` is itself tiny: with one output unit, here.)
    do_wrong = -c.out["g"] * wrong
    assert np.max(np.abs(do_wrong - fa["do"])) <= 1e-4 * max(1.0, np.max(np.abs(fa["do"])))
    print("    rel_err of the wrong form's do %.3e against closeness.py's bound %.3e"
          % (cl.rel_err(do_wrong, fa["do"]), cl.bound(cl.rel_err(f32["do"], fa["do"]))))


# ---- 2. the saturated target actor of the twin handle

def test_saturated_target_actor_clips_some_entries_and_leaves_others():
    c = sc.twin(*sc.TWIN_CASE)
    _, out, _ = sc.twin_step(c, c.eps)
    t_a = out["t_a"]
    at_clip, inside = int((np.abs(t_a) == 1.0).sum()), int((np.abs(t_a) < 1.0).sum())
    print("t_a: %d entries at +-1, %d inside" % (at_clip, inside))
    assert at_clip > 0 and inside > 0 and at_clip + inside == t_a.size == sc.B * c.A
    ho = o.actor_forward(c.target, c.batch[4])["ho"]
    assert np.mean(np.abs(ho) > sc.SATURATED) >= 0.10


# ---- 3. the saturated atom head

@pytest.mark.parametrize("S,A,N,k", sc.DIST_CASES)
def test_saturated_atom_head_conditions(S, A, N, k):
    c = sc.dist(S, A, N, k)
    p, pt = c.out["p"], c.out["pt"]
    rows_p, rows_pt = int((p < sc.SUBNORMAL).any(axis=1).sum()), int((pt < sc.SUBNORMAL).any(axis=1).sum())
    e_g = cl.rel_err(c.w32["g"], c.out["g"])
    e_row, _ = sc.ce_bound(c.w32["ce"], c.out["ce"])
    print("S=%d A=%d N=%d: p underflows in %d rows, p' in %d of %d; max p %.6f; logit spread %.0f; ce up to %.1f; e32(g) %.2e; ce per "
          "row e32 %.2e" % (S, A, N, rows_p, rows_pt, sc.B, p.max(), np.ptp(c.out["critic_fwd"]["logits"], axis=1).max(),
                            c.out["ce"].max(), e_g, e_row))
    assert 2 * rows_p >= sc.B and 2 * rows_pt >= sc.B
    assert p.max() > 0.999
    assert e_g <= 2.0 ** -10, "p (z - Q) cancels on a one-hot p: the bound on g would say nothing"
    assert np.all(np.isfinite(c.out["ce"])) and np.all(c.out["ce"] > 0)
    from test_gpu_dist import _kinds
    assert all(kind.any() for kind in _kinds(c.batch, N)), "done, clipped below, clipped above, done on an atom"
    for t in ("p", "dz", "ce", "g"):
        assert np.asarray(c.w32[t]).dtype == np.float32, t


# ---- 4. the shape limits

@pytest.mark.parametrize("S,A", sc.LIMITS)
def test_the_row_selection_finds_its_rows_at_the_limits(S, A):
    for c in (sc.actor(S, A), sc.twin(S, A), sc.dist(S, A, sc.LIMIT_ATOMS)):
        assert c.batch[0].shape == (sc.B, S) and c.batch[1].shape == (sc.B, A) and c.noise.shape == (A,)
    assert 2 * S + A + 2 == (162 if S == 64 else 5)
