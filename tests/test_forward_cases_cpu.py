"""The cases of tests/test_gpu_forward_relative.py without a GPU (tests/forward_cases.py builds them for both files): every
condition that makes them worth running, from the oracle and the restated launch rules alone.

  * SIZES holds both sides of every change of path(B) between 1 and 1025 rows and a size in each regime; the regimes are the
    eight of tests/README.md's table, and the sizes of the train form, the VALU net and the wide heads are among SIZES;
  * no compared tensor of the pool is all zero, every e32 is positive, the float32 run is float32 throughout (Side asserts it)
    and every bound is above closeness.FLOOR -- none is the floor's;
  * the policy is neither uniform nor saturated: row-max p within (0.15, 0.9) at A = 6, min p > 1e-6 at every head, so
    nothing sits near LOG_EPSILON; the continuous head's pool has no action near atan2's branch cut;
  * the batches: a permutation of the pool first; from 67 rows on every pool row, from 68 on at least one of them twice (the
    "same bits for copies" assertion has something to look at), from 512 on every one at least twice; never the same pool row
    twice in a row;
  * the structured rows' own tensors are non-zero, their bounds above the floor, and the five impulse frames differ from
    one another (and from the plain mid-grey relu(b1)) in n1.
"""
import numpy as np
import pytest

import closeness as c
import continuous_oracle as co
import forward_cases as fc
import ga3c_oracle as o


def test_sizes_hold_both_sides_of_every_change_of_the_launch_rules():
    assert fc.changes() == [129, 161, 177, 193, 257, 513, 1025]
    for b in fc.changes():
        assert b - 1 in fc.SIZES and b in fc.SIZES, b
    regimes = {fc.path(b) for b in range(1, fc.MAX_BATCH + 1)}
    assert regimes == {fc.path(b) for b in fc.SIZES} and len(regimes) == 8
    assert fc.path(1) == ("conv_stack_fwd", None, 16, "dense1_fwd_tile<1>") == fc.path(128)
    assert fc.path(129) == ("conv1_fwd+conv2_fwd", True, 22, "dense1_fwd_tile<2>") == fc.path(160)
    assert fc.path(161) == ("conv1_fwd+conv2_fwd", True, 22, "dense1_fwd<1>") == fc.path(176)
    assert fc.path(177) == ("conv1_fwd+conv2_fwd", True, 16, "dense1_fwd<1>") == fc.path(192)
    assert fc.path(193) == ("conv1_fwd+conv2_fwd", False, 16, "dense1_fwd<1>") == fc.path(256)
    assert fc.path(257) == ("conv1_fwd+conv2_fwd", False, 16, "dense1_fwd<2>") == fc.path(512)
    assert fc.path(513) == ("conv1_fwd+conv2_fwd", False, 8, "dense1_fwd<2>") == fc.path(1024)
    assert fc.path(1025) == ("conv1_fwd+conv2_fwd", False, 4, "dense1_fwd<2>")
    # the reasons the table gives: 240 and 288 workgroups of the tile kernel at 160 | 161 rows, 164,352 B of LDS at 177
    assert 8 * 5 * 6 == 240 and 8 * 6 * 6 == 288 > 256 and (16 * 8 * 256 + 32 * fc.D1F_AS) * 4 == 164352 > 160 * 1024
    # GA3C_D1F_TILE=0: dense1_fwd<1> to 256 rows, <2> beyond, at the same slice counts
    assert all(fc.path(b, False)[:3] == fc.path(b)[:3] for b in fc.SIZES)
    assert all(fc.path(b, False)[3] == "dense1_fwd<%d>" % (1 if b <= 256 else 2) for b in fc.SIZES)
    # the tile edges: 16 rows per tile, 32 per workgroup of the two-tile kernels
    assert {15, 16, 17, 144, 145} <= set(fc.SIZES) and 144 % 16 == 0 and 160 % 32 == 0
    assert len(fc.SIZES) == len(set(fc.SIZES)) == 22 and max(fc.SIZES) == fc.MAX_BATCH
    for sizes in (fc.TRAIN_SIZES, fc.VALU_SIZES, fc.WIDE_SIZES, fc.STRUCTURED_SIZES):
        assert set(sizes) <= set(fc.SIZES)
    assert {fc.path(b)[0] for b in fc.TRAIN_SIZES} == {"conv_stack_fwd", "conv1_fwd+conv2_fwd"}
    assert {fc.dense_ks(b) for b in fc.VALU_SIZES} == {22, 16, 8, 4} and {fc.dense_ks(b) for b in fc.WIDE_SIZES} == {16, 8, 4}


def test_the_pool_is_the_one_the_cases_describe():
    xk, x = fc.pool()
    assert xk.shape == (fc.R, 84, 84, 4) and xk.dtype == np.uint8 and x.dtype == np.float32 and fc.R == 67
    assert not xk[fc.ZEROS].any() and np.all(xk[fc.ONES] == 255) and np.all(x[fc.ZEROS] == -1.0)
    for i, (row, col) in enumerate(fc.IMPULSES):
        frame = x[fc.IMPULSE0 + i]
        assert np.count_nonzero(frame) == 4 and np.all(frame[row, col] == np.float32(255 / 128.0 - 1.0))
    assert len({xk[i].tobytes() for i in range(fc.R)}) == fc.R
    assert np.array_equal(x, xk.astype(np.float32) / np.float32(128.0) - np.float32(1.0))


@pytest.mark.parametrize("head,num_actions", [("disc", fc.A)] + list(fc.WIDE))
def test_no_compared_tensor_is_all_zero_and_every_bound_is_above_the_floor(head, num_actions):
    s = fc.side(head, num_actions)
    assert set(s.want) == set(fc.NAMES if num_actions == fc.A else fc.OUT_NAMES)
    for name, want in s.want.items():
        assert want.shape[0] == fc.R and np.any(want) and s.scale[name] > 0, name
        assert s.e32[name] > 0.0 and c.FLOOR < s.bound(name) < 1e-4, (name, s.e32[name])
        assert np.all(np.any(want != want[0], axis=1)[1:]), name             # every row's tensor differs from the first row's
        print("%s A=%d %-3s max|T| %.3e  e32 %.3e  bound %.3e" % (head, num_actions, name, s.scale[name], s.e32[name], s.bound(name)))
    for k, v in fc.params(head, num_actions).items():
        assert np.array_equal(v, v.astype(np.float32)), k                    # the arena holds these values exactly
    p = s.want["p"]
    if head == "disc":
        assert np.max(np.abs(p.sum(axis=1) - 1.0)) < 1e-14 and p.min() > 1e-6
        print("%s A=%d: row-max p %.3f .. %.3f, min p %.2e, max|z| %.2f" % (head, num_actions, p.max(axis=1).min(),
                                                                          p.max(axis=1).max(), p.min(), s.scale["z"]))
        if num_actions == fc.A:
            assert 0.15 < p.max(axis=1).min() and p.max(axis=1).max() < 0.9
            assert s.scale["z"] > 1.0                                            # (0.1 with the seeded weights)
        else:
            assert p.max() > 4.0 / num_actions                                   # not uniform either
    else:
        _, x = fc.pool()
        f = co.forward(fc.params(head, num_actions), x.astype(np.float64), keep=True)
        cut = f["X"] < 0
        # atan2's branch cut: a float32 Y (error 1e-7) cannot change sign anywhere, and no radius is near zero
        assert np.min(np.abs(f["Y"][cut])) > 1e-5 and np.min(f["X"] ** 2 + f["Y"] ** 2) > 1e-6
        assert np.all(np.abs(p) < 1.0)


def test_the_weights_differ_from_the_seeded_ones_in_the_policy_head_only():
    seeded, mine = o.init_params(fc.A), fc.params("disc", fc.A)
    for k in o.PARAM_ORDER:
        want = np.asarray(seeded[k]) * (fc.P_SCALE if k == "logits_p/w" else 1.0)
        assert np.array_equal(mine[k], want.astype(np.float32).astype(np.float64)), k
    uniform = o.forward(seeded, fc.pool()[1].astype(np.float64))
    assert uniform["p"].max() < 0.2 and np.abs(uniform["z"]).max() < 0.2     # what the older forward tests look at


@pytest.mark.parametrize("bsz", fc.SIZES)
def test_the_batches_are_permutations_of_the_pool_with_draws_behind(bsz):
    idx = fc.index(bsz)
    count = np.bincount(idx, minlength=fc.R)
    assert idx.shape == (bsz,) and idx.min() >= 0 and idx.max() < fc.R
    assert np.all(np.bincount(idx[:fc.R], minlength=fc.R) <= 1)              # the head of the batch: a permutation
    assert not np.any(idx[1:] == idx[:-1])
    if bsz >= fc.R:
        assert count.min() >= 1
    if bsz > fc.R:
        assert count.max() >= 2
    if bsz >= 127:
        assert np.sum(count >= 2) > fc.R // 2
    if bsz >= 512:
        assert count.min() >= 2
    if bsz > 1:
        assert not np.array_equal(idx, np.sort(idx))                         # and not the pool's own order
    _, xk, x = fc.rows(bsz)
    assert xk.shape == (bsz, 84, 84, 4) and xk.flags.c_contiguous and x.flags.c_contiguous
    a, y = fc.targets(bsz)
    assert a.shape == (bsz, fc.A) and np.all(a.sum(axis=1) == 1) and y.shape == (bsz,)


def test_the_structured_rows_have_tensors_of_their_own():
    s, pool = fc.structured(), fc.side()
    for name in fc.NAMES:
        assert s.want[name].shape[0] == 7 and np.any(s.want[name]) and s.e32[name] > 0.0, name
        assert c.FLOOR < s.bound(name) < 1e-4 and s.scale[name] <= pool.scale[name], name
        print("structured %-3s max|T| %.3e (pool %.3e)  e32 %.3e  bound %.3e" % (name, s.scale[name], pool.scale[name],
                                                                                 s.e32[name], s.bound(name)))
    assert s.scale["n1"] < 0.75 * pool.scale["n1"]                           # the pool's scale would hide their n1
    # a mid-grey frame is x = 0: n1 = relu(b1) in every pixel; each impulse moves its own corner of n1, and no two alike
    b1 = np.maximum(fc.params("disc", fc.A)["conv11/b"], 0)
    n1 = s.want["n1"][fc.IMPULSE0 - fc.RANDOM:].reshape(5, 21, 21, 16)
    for i in range(5):
        moved = np.any(n1[i] != b1, axis=-1)
        assert 1 <= moved.sum() <= 4, (i, int(moved.sum()))                  # an 8 x 8 filter at stride 4 sees a pixel from <= 4 outputs
        for j in range(i):
            assert np.any(n1[i] != n1[j]), (i, j)
    corners = [tuple(np.argwhere(np.any(n1[i] != b1, axis=-1))[0]) for i in range(4)]
    assert corners == [(0, 0), (0, 20), (20, 0), (20, 20)]
    for bsz in fc.STRUCTURED_SIZES:
        idx = fc.structured_index(bsz)
        assert idx.shape == (bsz,) and set(fc.STRUCTURED) <= set(idx) and not np.any(idx[1:] == idx[:-1]), bsz


def test_scaled_divides_by_the_pools_scale():
    got, want = fc.scaled([0.5, 1.0], [0.5, 0.75], 4.0)
    assert c.rel_err(got, want) == 0.25 / 4.0 and c.rel_err([0.5, 1.0], [0.5, 0.75]) == 0.25 / 0.75
    with pytest.raises(AssertionError):
        fc.scaled([1.0], [5.0], 4.0)
