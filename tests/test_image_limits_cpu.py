"""The cases of tests/test_gpu_image_limits.py without a GPU (tests/image_limit_cases.py builds them for both files): every
condition that makes them worth running, from the oracles alone.

  * the shapes are the ones the issue names: both sides of launch_heads' seams (8 | 9 and 24 | 25 policy columns, 2A of them
    under CONTINUOUS_INPUT), the limit, an odd stride next to it; every A meets B = 1 and 17, the limit shapes 97, 121 and 129;
  * no compared tensor of the float64 oracle is all zero but the documented ones (dz, logits_p/* at A = 1; under dual the
    tensors a cost cannot reach), those are zero in float32 too, and e32 > 0 for every other compared tensor;
  * the float32 runs that supply e32 stay in float32 (continuous_oracle.loss_and_grads used to cast y_r and a to float64);
  * the continuous rows: safe_rows' rule and the floor X^2 + Y^2 >= 1e-5 together keep at least 60 % of the candidates, the
    main cases hold no row below the floor and the two `near` cases hold at least three;
  * the second step, held to the oracle like the first, starts from weights at which every tensor is still alive: the oracle's
    own first step at LR_SMALL leaves such weights, one at LR_PROBE would not;
  * the saturated policy at A = 25 and 64: min p < 1e-9, max p > 0.9999, 0.1 < clamped share < 0.9, at least 4 of 32 rows on
    each side of the clamp for the selected action, and no p within 1 % of LOG_EPSILON.
"""
import numpy as np
import pytest

import closeness as c
import continuous_oracle as co
import dual_oracle as d
import ga3c_oracle as o
import image_limit_cases as ic


def test_the_shapes_are_the_ones_the_dispatcher_and_the_create_call_turn_on():
    amax = lambda npc: 8 if npc <= 8 else 24 if npc <= 24 else 64        # launch_heads (ga3c_engine.hip)
    assert [amax(A) for A in ic.ACTIONS["disc"]] == [8, 8, 24, 24, 64, 64, 64]
    assert [amax(2 * A) for A in ic.ACTIONS["cont"]] == [8, 24, 24, 64, 64, 64]
    assert [amax(A) for A in ic.ACTIONS["dual"]] == [24, 64, 64]
    assert max(ic.ACTIONS["disc"]) == 64 and max(ic.ACTIONS["cont"]) == 32         # GA3C_MAX_ACTIONS and half of it
    for head in ic.HEADS:
        for A in ic.ACTIONS[head]:
            assert set(ic.sizes(head, A)) >= {1, 17}
            assert (set(ic.sizes(head, A)) >= {97, 121, 129}) == (A in ic.LIMIT[head])
            assert max(ic.sizes(head, A)) <= ic.MAX_BATCH
    assert len(ic.CASES) == len(set(ic.CASES)) == 20 + 15 + 9


@pytest.mark.parametrize("head,num_actions,bsz,near", [k + (False,) for k in ic.CASES] + [("cont", A, B, True) for A, B in ic.NEAR])
def test_no_compared_tensor_is_all_zero_and_every_e32_is_positive(head, num_actions, bsz, near):
    cs = ic.case(head, num_actions, bsz, near)
    fc = ic.forward_case(head, num_actions, bsz, near=near)
    zeros = ic.zero_tensors(head, num_actions)
    for name in cs.tensors:
        assert np.asarray(cs.g32[name]).dtype == np.float32, name
        if name in zeros:
            assert not np.any(cs.g[name]) and not np.any(cs.g32[name]) and cs.e32[name] == 0.0, name
        else:
            assert np.any(cs.g[name]) and cs.e32[name] > 0.0, (name, cs.e32[name])
            assert ic.bound(cs, name, np.size(cs.g[name])) < 1e-3, (name, cs.e32[name])     # a bound that still says something
    for name in ("p", "v", "z"):
        assert np.any(fc.want[name]), name
        if head == "disc" and num_actions == 1 and name == "p":
            assert np.all(fc.want["p"] == 1.0) and fc.e32["p"] == 0.0       # one action: p = 1 in every precision
        elif not (fc.want[name].size == 1 and fc.e32[name] == 0.0):         # a single draw may come out exact: the floor holds it
            assert fc.e32[name] > 0.0, name
    if head == "disc":
        assert np.max(np.abs(fc.want["p"].sum(axis=1) - 1.0)) < 1e-14
    print("%s A=%d B=%d%s: largest e32 %.2e (%s)" % (head, num_actions, bsz, " near" if near else "",
                                                      max(cs.e32.values()), max(cs.e32, key=cs.e32.get)))


@pytest.mark.parametrize("num_actions,bsz", ic.NEAR)
def test_the_near_cases_hold_rows_below_the_floor(num_actions, bsz):
    below, rmin = ic.rows_below_floor(num_actions, bsz)
    main = ic.case("cont", num_actions, bsz)
    near = ic.case("cont", num_actions, bsz, True)
    print("cont A=%d B=%d near: %d rows below the floor, smallest radius %.2e; e32(dz) %.2e against %.2e with the floor"
          % (num_actions, bsz, below, rmin, near.e32["dz"], main.e32["dz"]))
    assert below >= ic.NEAR_MIN_ROWS and rmin >= ic.MIN_ABS_Y


@pytest.mark.parametrize("num_actions", ic.ACTIONS["cont"])
def test_safe_rows_and_the_floor_keep_the_continuous_batches(num_actions):
    p = ic.params("cont", num_actions)
    for bsz in ic.sizes("cont", num_actions):
        kept, total = ic.cont_kept(num_actions, bsz)
        assert total == 2 * bsz + 16 and kept >= ic.MIN_KEPT * total, (num_actions, bsz, kept, total)
        _, x, a, y = ic.rows("cont", num_actions, bsz)
        assert x.shape[0] == bsz and a.shape == (bsz, num_actions) and a.dtype == np.float32
        f = co.forward(p, x.astype(np.float64), keep=True)
        assert np.all(f["X"] ** 2 + f["Y"] ** 2 >= ic.FLOOR_R2) and co.safe_rows(p, x.astype(np.float64), ic.MIN_ABS_Y).all()
        print("cont A=%d B=%d: both rules keep %d of %d candidate rows (%.0f %%)" % (num_actions, bsz, kept, total,
                                                                                      100.0 * kept / total))


def test_the_oracles_stay_in_float32_when_handed_float32():
    """e32 would be a lower limit only if a float32 run left float32 anywhere.  continuous_oracle.loss_and_grads cast y_r, a
    and adv_const to float64 (every tensor behind the loss came out float64): it follows the dtype of x / params now."""
    for head, A in (("cont", 5), ("dual", 9)):
        _, x, a, y = ic.rows(head, A, 1)
        p32 = c.f32_params(ic.params(head, A))
        if head == "cont":
            losses, g = co.loss_and_grads(p32, x, y, a, ic.BETA)
            out = dict(g)
        else:
            losses, gp, gv = d.dual_grads(p32, x, y, a, ic.BETA)
            out = {"p:" + k: v for k, v in gp.items()}
            out.update({"v:" + k: v for k, v in gv.items()})
        for k, v in out.items():
            assert np.asarray(v).dtype == np.float32, (head, k, np.asarray(v).dtype)
        assert all(np.asarray(v).dtype == np.float32 for v in losses.values()), head


def test_relu_on_of_the_two_oracles_is_the_identity_at_their_own_units():
    """relu_on (new in continuous_oracle and dual_oracle) handed the oracle's own units changes nothing; one unit switched
    changes dd1 in that unit alone."""
    for head, A in (("cont", 4), ("dual", 9)):
        cs = ic.case(head, A, 17)
        same = cs._grads(cs.on)[1]
        assert all(np.array_equal(same[k], cs.g[k]) for k in cs.tensors), head
        on = {k: v.copy() for k, v in cs.on.items()}
        on["d1"][3, 7] = not on["d1"][3, 7]
        other = cs._grads(on)[1]
        name = "dd1" if head == "cont" else "p:dd1"
        diff = other[name] != cs.g[name]
        assert diff[3, 7] and diff.sum() == 1, head


@pytest.mark.parametrize("head", ic.HEADS)
def test_the_second_step_starts_from_weights_at_which_every_tensor_is_alive(head):
    """The GPU file's second step is compared against the oracle at the device's theta'.  Here: the oracle's own first step
    at LR_SMALL (plain and clipped) leaves weights at which no compared tensor is all zero and e32 is of the usual size --
    and a first step at LR_PROBE would not: the continuous head's float32 oracle then loses a tensor altogether."""
    A = max(ic.ACTIONS[head])
    for variant in ("plain",) if head == "dual" else ("plain", "clip"):
        for bsz in (17, 129):
            _, x, a, y = ic.rows(head, A, bsz)
            cs = ic.make_case(head, ic.oracle_theta1(head, A, bsz, variant), x, y, a)
            for name in cs.tensors:
                if name not in ic.zero_tensors(head, A):
                    assert np.any(cs.g[name]) and 0.0 < cs.e32[name] < 1e-4, (variant, bsz, name, cs.e32[name])
            print("%s A=%d B=%d after one %s step at lr %g: largest e32 %.2e (%s)" % (
                head, A, bsz, variant, ic.LR_SMALL, max(cs.e32.values()), max(cs.e32, key=cs.e32.get)))
    if head == "cont":
        _, x, a, y = ic.rows(head, A, 17)
        with np.errstate(over="ignore"):
            cs = ic.make_case(head, ic.oracle_theta1(head, A, 17, "plain", ic.LR_PROBE), x, y, a)
        assert max(cs.e32.values()) > 1e-4


@pytest.mark.parametrize("num_actions", ic.SOFTMAX_A)
def test_the_three_softmax_settings_differ_where_they_should(num_actions):
    fs = {k: ic.forward_case("disc", num_actions, ic.SOFTMAX_B, k) for k in ic.SOFTMAX}
    assert np.array_equal(fs["default"].want["p"], fs["log_softmax"].want["p"])          # USE_LOG_SOFTMAX changes the loss only
    s = fs["default"].want["p"]
    assert np.allclose(fs["min_policy"].want["p"], (s + 0.01) / (1.0 + 0.01 * num_actions), rtol=0, atol=1e-15)
    assert np.max(np.abs(fs["min_policy"].want["p"] - s)) > 1e-4        # a hundred times the bound the GPU file holds p to
    assert np.max(np.abs(fs["min_policy"].want["p"].sum(axis=1) - 1.0)) < 1e-14


@pytest.mark.parametrize("num_actions", sorted(ic.SATURATED))
def test_the_saturated_policy_is_saturated_at_the_wide_heads(num_actions):
    s = ic.check_saturated(num_actions)
    print("saturated A=%d seed %d: clamped share %.2f, %d / %d rows with the selected action clamped / open, nearest p to "
          "LOG_EPSILON %.1f %% away, min p %.1e, max p %.6f" % (num_actions, ic.SATURATED[num_actions], s["share"],
                                                               s["clamped_rows"], s["open_rows"], 100 * s["nearest"],
                                                               s["min_p"], s["max_p"]))
    p, _, x, a, y = ic.saturated(num_actions)
    for kw in ({}, dict(use_log_softmax=True)):
        _, g = o.loss_and_grads(p, x.astype(np.float64), y, a.astype(np.float64), 0.01, **kw)
        assert all(np.any(g[k]) and np.all(np.isfinite(g[k])) for k in c.TENSORS), kw


def test_the_variable_layout_the_plumbing_test_expects():
    """ga3c_net_param_info is checked against these offsets: PARAM_ORDER, each tensor after the one before."""
    for head, A in (("disc", 64), ("cont", 32)):
        off = {}
        n = 0
        for k in ic.order(head):
            off[k] = n
            n += int(np.prod(ic.shapes(head, A)[k]))
        assert n == ic.flat(head, ic.params(head, A)).size
        if head == "disc":
            assert n == o.param_count(64) and off["logits_p/b"] - off["logits_p/w"] == 256 * 64
        else:
            assert [off[k] - off["logits_p/out_x/w"] for k in co.HEADS] == [0, 256 * 32, 257 * 32, 513 * 32]
