"""The cases of tests/test_gpu_backward_seams.py without a GPU (tests/backward_cases.py builds them for both files): every
condition that makes them worth running, from the oracle and the restated launch rules alone.

  * SIZES holds both sides of every change of regime(B) between 161 and 1025 rows and a size in each regime; every trip count
    of bwd_path(B) that changes at a size SIZES does not hold is one more trip of a loop that SIZES already runs at a smaller
    and at a larger count (the sixth to eighth 128-row chunk, the fourth conv2_dw pass, the units of a conv1_dw workgroup);
  * the constants restated in backward_cases.py are those of the source, read from its text;
  * the composed float64 tensors equal o.loss_and_grads on the materialised batch, the composed float32 tensors are float32;
  * no compared tensor is all zero, every e32 is positive, every bound above closeness.FLOOR;
  * one past a boundary the last row's entry differs from the entries a dropped or doubled pass would confuse it with;
  * closeness.signed_or_magnitude's cap holds on the oracle at every size;
  * the float32 composition in the batch's order and in the kernels' slab order at 1025 rows: their ratio per tensor.
"""
import os
import re

import numpy as np
import pytest

import backward_cases as bc
import closeness as c
import forward_cases as fc
import ga3c_oracle as o

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ga3c_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def test_sizes_hold_both_sides_of_every_change_of_the_launch_rules():
    assert bc.changes(bc.regime) == [177, 193, 257, 513, 1025]
    for b in bc.changes(bc.regime):
        assert b - 1 in bc.SIZES and b in bc.SIZES, b
    regimes = {bc.regime(b) for b in range(161, bc.MAX_BATCH + 1)}
    assert regimes == {bc.regime(b) for b in bc.SIZES} and len(regimes) == 6
    # which rule changes where
    p = bc.bwd_path
    assert (p(192).gather, p(193).gather) == ("args", "pinned")
    assert (p(256).conv, p(257).conv) == ("pair", "split") and (p(256).nch1, p(257).nch1) == (256, 512)
    assert [p(b).nch2 for b in (255, 256, 257, 1025)] == [255, 256, 256, 256]
    assert [p(b).c2dw_passes for b in (256, 257, 512, 513, 1024, 1025)] == [1, 2, 2, 3, 4, 5]
    assert [p(b).c1dw_units for b in (256, 257)] == [7, 4] and 7 * 257 // 512 == 3            # three to four units each
    assert [(p(b).chunks, p(b).last_rows) for b in (256, 257, 384, 385, 512, 513, 1024, 1025)] == \
        [(2, 128), (3, 1), (3, 128), (4, 1), (4, 128), (5, 1), (8, 128), (9, 1)]
    assert [p(b).wide_b_passes for b in (1024, 1025)] == [1, 2] and [p(b).wide_w_passes for b in (256, 257, 1025)] == [2, 3, 9]
    assert not any(p(b).tail for b in bc.SIZES) and all(p(b).tail for b in range(129, 134)) and not p(134).tail
    assert all(p(b).defer_wd and p(b).c2dx_grid == b + 121 for b in bc.SIZES)
    assert all(p(b).forward == fc.path(b) for b in bc.SIZES)
    # the trip counts: a change that SIZES does not straddle is one more trip of a loop SIZES runs at fewer and at more trips
    for field in bc.LOOP_FIELDS:
        held = {getattr(p(b), field) for b in bc.SIZES}
        for b in bc.changes(lambda n: getattr(p(n), field)):
            if b - 1 in bc.SIZES and b in bc.SIZES:
                continue
            trips = getattr(p(b), field)
            assert min(held) < trips < max(held) or trips in held, (field, b, trips)
            assert bc.regime(b) == bc.regime(b - 1) or b in bc.SIZES, (field, b)
    assert [b for b in bc.changes(lambda n: p(n).chunks) if b not in bc.SIZES] == [641, 769, 897]
    assert set(bc.ONE_PAST) <= set(bc.SIZES) and all(p(b).last_rows == 1 for b in bc.ONE_PAST if b != 193)
    assert len(bc.SIZES) == 14 and max(bc.SIZES) == bc.MAX_BATCH
    for sizes in (bc.WIDE_SIZES, bc.LAST_ROW_SIZES, bc.GATHER_SIZES, tuple(bc.HEAVY_ROWS)):
        assert set(sizes) <= set(bc.SIZES)
    for bsz, rows in bc.HEAVY_ROWS.items():       # first row, last row of the last full chunk, last row
        assert {0, (bsz - 1) // 128 * 128 - 1, bsz - 1} <= set(rows), bsz


def test_the_restated_constants_are_the_sources():
    eng, ker = _source("ga3c_engine.hip"), _source("ga3c_kernels.hpp")

    def const(text, name):
        return int(re.search(r"\b%s = (\d+)" % name, text).group(1))
    assert const(eng, "DW_PAIR_MAX_B") == bc.DW_PAIR_MAX_B
    assert (const(eng, "CONV_BWD_MIN_B"), const(eng, "CONV_BWD_MAX_B")) == (bc.CONV_BWD_MIN_B, bc.CONV_BWD_MAX_B)
    assert const(eng, "FUSED_CONV_MAX_B") == 128 and const(eng, "C2F_QUARTER_MAX_B") == 192
    assert (const(ker, "D1B_ROWS"), const(ker, "D1B_TAIL_ROWS")) == (bc.D1B_ROWS, bc.D1B_TAIL_ROWS)
    assert re.search(r"C2DX_WD_BLOCKS = KSTEPS_DENSE / 2;", ker) and re.search(r"KSTEPS_DENSE = FLAT / 16;", ker)
    assert o.FLAT // 16 == fc.KSTEPS_DENSE and bc.C2DX_WD_BLOCKS == 121
    # rules the source writes as literals
    assert re.search(r"if \(B <= %d && net->offsets_in_args\)" % bc.GATHER_ARGS_MAX_B, eng)
    assert re.search(r"return \{conv1_dw_blocks\(B\), B < 256 \? B : 256, false\};", eng)
    assert re.search(r"int n = 512;\s+if \(B <= 256\) \{\s+const int one_round = 768 - 4 \* B;\s+n = 5 \* one_round >= units \? one_round : 256;", eng)
    assert re.search(r"for \(int b0 = bg; b0 < h\.B; b0 \+= 128\)", ker) and len(re.findall(r"b < h\.B; b \+= 1024\)", ker)) == 2
    assert re.search(r"for \(int c0 = 0; c0 < B - trows; c0 \+= D1B_ROWS\)", ker)
    assert re.search(r"d\.tail_lds = B > D1B_ROWS && B <= D1B_ROWS \+ D1B_TAIL_ROWS;", eng)
    assert re.search(r"upd\.defer_wd = upd\.on && \(!fused_cb \|\| 2 \* B >= KSTEPS_DENSE\);", eng)
    assert re.search(r"dim3\(B \+ C2DX_WD_BLOCKS, 2\)", eng)


def test_the_entries_are_the_ones_the_cases_describe():
    ent = bc.entries()
    assert ent.state.shape == (70,) and np.array_equal(ent.state[:bc.R], np.arange(bc.R)) and tuple(ent.state[bc.R:]) == bc.HEAVY_STATES
    assert ent.y.dtype == np.float32 and np.all(np.abs(ent.y[:bc.R]) < 1) and np.all(np.abs(ent.y[bc.R:]) == bc.HEAVY_Y)
    assert ent.a.shape == (70, bc.A) and np.all(ent.a.sum(axis=1) == 1) and set(np.argmax(ent.a[:bc.R], axis=1)) == set(range(bc.A))
    assert all(s < fc.RANDOM for s in bc.HEAVY_STATES)
    for bsz in bc.SIZES:
        assert index_max(bsz) < bc.R                      # no plain batch holds a heavy entry
    idx = bc.index_with(257, 255, bc.HEAVY[1])
    assert idx[255] == bc.HEAVY[1] and np.array_equal(np.delete(idx, 255), np.delete(bc.index(257), 255))
    xk, x, y, a = bc.batch(idx)
    assert xk.shape == (257, 84, 84, 4) and abs(y[255]) == 100 and np.array_equal(xk[255], fc.pool()[0][bc.HEAVY_STATES[1]])


def index_max(bsz):
    return int(bc.index(bsz).max())


@pytest.mark.parametrize("bsz", [161, 257])
def test_the_composed_tensors_are_the_oracles_on_the_materialised_batch(bsz):
    s = bc.side()
    idx = bc.index_with(bsz, bsz - 1, bc.HEAVY[0]) if bsz == 257 else bc.index(bsz)      # (one of them with a heavy row)
    _, x, y, a = bc.batch(idx)
    losses, g = o.loss_and_grads(s.params, x.astype(np.float64), y.astype(np.float64), a.astype(np.float64), bc.BETA)
    got = s.compose64(idx)
    worst = 0.0
    for name in c.TENSORS:
        assert got[name].shape == np.asarray(g[name]).reshape(got[name].shape).shape
        err = c.rel_err(got[name], g[name])
        worst = max(worst, err)
        assert err <= 1e-12, (name, err)
    for i, name in enumerate(bc.LOSSES):
        assert abs(got["loss"][i] - losses[name]) <= 1e-12 * abs(losses[name]), name
    print("B=%d: composed against materialised, worst rel_err over the fifteen tensors %.1e" % (bsz, worst))
    for name, t in s.compose32(idx).items():
        assert t.dtype == np.float32, name
    for name, t in s.compose32(idx, 256).items():
        assert t.dtype == np.float32, name


def test_the_units_of_a_counterpart_reach_the_composition():
    """want(idx, on) with the oracle's own units is the plain composition; with the float32 run's units it is e32's reference;
    copies of an entry that disagree, and a unit far from zero switched, are refused."""
    s = bc.side()
    idx = bc.index(161)
    own = {k: s.on[k][s.ent.state[idx]] for k in c.ACTS}
    plain = s.compose64(idx)
    assert all(np.array_equal(s.want(idx, own)[k], plain[k]) for k in c.TENSORS)
    on32 = {k: s.on32[k][s.ent.state[idx]] for k in c.ACTS}
    ref = s.compose64(idx, s.ref32[0])
    got = s.want(idx, on32)
    assert all(np.array_equal(got[k], ref[k]) for k in c.TENSORS)
    print("float32 run: %d unit(s) of the 70 entries differ from the float64 run's" % s.ref32[1])
    twice = int(np.flatnonzero(np.bincount(idx) >= 2)[0])
    bad = {k: v.copy() for k, v in own.items()}
    row = np.flatnonzero(idx == twice)[1]
    bad["d1"][row] = ~bad["d1"][row]
    with pytest.raises(AssertionError, match="copies of a pool entry"):
        s.want(idx, bad)
    far = {k: v.copy() for k, v in own.items()}
    rows = np.flatnonzero(idx == twice)
    unit = int(np.argmax(np.abs(s.pre["d1"][twice])))
    far["d1"][rows, unit] = ~far["d1"][rows, unit]
    with pytest.raises(AssertionError, match="switched the other way"):
        s.want(idx, far)


def test_units_within_rounding_of_zero_are_evaluated_as_handed_over():
    """Neither the float32 oracle nor the MI355X switched a unit of these 70 entries, so the re-evaluation is run here: in each
    layer the unit of the pool whose input is nearest zero (all three lie within the condition's limit) switched in every copy of
    its state.  The composition must equal o.loss_and_grads(relu_on=) on the materialised batch, and differ from the plain one."""
    s = bc.side()
    idx = bc.index(161)
    _, x, y, a = bc.batch(idx)
    on = {k: s.on[k][s.ent.state[idx]].copy() for k in c.ACTS}
    for k in c.ACTS:
        state, unit = np.unravel_index(np.argmin(np.abs(s.pre[k])), s.pre[k].shape)
        assert abs(s.pre[k][state, unit]) <= c.bound(s.act_e32[k], k) * s.pre_scale[k], k
        rows = np.flatnonzero(idx == state)
        assert rows.size >= 1
        on[k][rows, unit] = ~on[k][rows, unit]
    got, plain = s.want(idx, on), s.compose64(idx)
    f = o.forward(s.params, x.astype(np.float64), keep=True)
    _, g = o.loss_and_grads(s.params, x.astype(np.float64), y.astype(np.float64), a.astype(np.float64), bc.BETA,
                            relu_on={k: on[k].reshape(f[k].shape) for k in c.ACTS}, f=f)
    for name in c.TENSORS:
        assert c.rel_err(got[name], g[name]) <= 1e-12, name
    assert any(np.any(got[name] != plain[name]) for name in ("dn1", "dn2", "dd1"))


@pytest.mark.parametrize("bsz", bc.SIZES)
def test_no_compared_tensor_is_all_zero_and_every_bound_is_above_the_floor(bsz):
    s = bc.side()
    idx = bc.index(bsz)
    want = s.compose64(idx)
    e32, loss = s.e32(idx)
    for name in c.TENSORS:
        assert np.any(want[name]) and e32[name] > 0.0, name
        assert c.FLOOR < bc.bound(e32, name, bsz) < 1e-4, (name, e32[name])
    assert all(0.0 < e < 1e-4 / 16 for e in loss), loss           # 16 x e stays under the rtol of 1e-4 the sums are held to as well
    for name in c.ACTS:
        assert c.FLOOR < c.bound(e32[name], name) < 1e-4, name
    # signed_or_magnitude's cap, on the oracle alone: under 1 % of a tensor's entries too small to carry a sign
    for name in o.PARAM_ORDER:
        c.signed_or_magnitude(np.sign(want[name]), np.abs(want[name]), want[name])


@pytest.mark.parametrize("bsz", bc.SIZES)
def test_the_last_rows_entry_differs_from_the_rows_a_slipped_pass_would_confuse_it_with(bsz):
    idx = bc.index(bsz)
    for back in range(128, bsz, 128):
        assert idx[-1] != idx[bsz - 1 - back], (bsz, back)
    assert idx[-1] != idx[0] and idx[-1] != idx[-2]
    assert np.array_equal(idx[:-1], fc.index(bsz)[:-1]) and (idx[-1] == fc.index(bsz)[-1]) == (bsz not in (161, 192, 384))
    assert fc.index(384)[383] == fc.index(384)[127]               # what bc.index moves on
    # ... and its terms are not small beside the sums they enter: dropping the row moves every gradient by more than its bound
    s = bc.side()
    e32, _ = s.e32(idx)
    full, short = s.compose64(idx), s.compose64(idx[:-1])
    for name in o.PARAM_ORDER:
        moved = float(np.max(np.abs(full[name] - short[name]))) / float(np.max(np.abs(full[name])))
        assert moved > 4 * bc.bound(e32, name, bsz), (name, moved, bc.bound(e32, name, bsz))


def test_the_heavy_and_the_last_row_batches():
    s = bc.side()
    for bsz, rows in bc.HEAVY_ROWS.items():
        for i, row in enumerate(rows):
            idx = bc.index_with(bsz, row, bc.HEAVY[i % 3])
            want = s.compose64(idx)
            e32, _ = s.e32(idx)
            assert abs(want["dv"][row]) > 90 and np.max(np.abs(np.delete(want["dv"], row))) < 3          # the row dominates
            # (dv = v - y at |y| = 100 is exact to an ulp of 100 in either precision: 16 x e32 is 5e-7 and the floor holds it)
            assert all(e32[k] > 0 and c.FLOOR < bc.bound(e32, k, bsz) < 1e-4 for k in c.TENSORS if k != "dv"), (bsz, row)
            assert 0 < e32["dv"] and bc.bound(e32, "dv", bsz) == c.FLOOR
    q, qidx = bc.last_row_side()
    for bsz in bc.LAST_ROW_SIZES:
        idx = qidx[bsz]
        assert idx.shape == (bsz,) and idx[-1] >= bc.R and np.array_equal(idx[:-1], bc.index(bsz)[:-1])
        want = q.compose64(idx)
        e32, loss = q.e32(idx)
        assert np.max(np.abs(want["dv"][:-1])) < 2.0 ** -24 * 4 < 1e-3 < abs(want["dv"][-1])      # the others: the rounding of v
        assert loss[1] == 0.0 and want["loss"][1] == 0.0                                             # beta = 0
        # (dz and dv are one row's: a rounding or two of p and v, 16 x e32 = 6e-7 .. 2e-6, and the floor holds dv at every size)
        assert all(np.any(want[k]) and e32[k] > 0 and c.FLOOR < bc.bound(e32, k, bsz) < 1e-4 for k in c.TENSORS[2:]), bsz
        assert 0 < e32["dz"] and 0 < e32["dv"] and bc.bound(e32, "dv", bsz) == c.FLOOR


def test_two_summation_orders_of_the_float32_composition_at_1025_rows():
    """The batch's order (row after row: what e32 is taken from) against the kernels' slab order (partial sums over 256 and
    512 groups, then a tree; dense1/w chunk by chunk): rel_err of each against the float64 composition, and their ratio.  The
    slab order is the more accurate one in every tensor -- shorter chains --, so 16 x e32 of the batch order is no tighter for
    a kernel that sums in slabs than it is at 160 rows: the evidence for leaving SIZE_FACTOR empty."""
    s = bc.side()
    idx = bc.index(1025)
    ref = s.compose64(idx, s.ref32[0], "ref32")
    rows = s.compose32(idx)
    for groups in (256, 512):
        slabs = s.compose32(idx, groups)
        for name in o.PARAM_ORDER:
            e_rows, e_slabs = c.rel_err(rows[name], ref[name]), c.rel_err(slabs[name], ref[name])
            print("1025 rows, %3d groups  %-12s batch order %.2e  slab order %.2e  ratio %.2f" % (groups, name, e_rows, e_slabs,
                                                                                                e_slabs / e_rows))
            assert e_slabs <= c.FACTOR * e_rows, (name, e_slabs, e_rows)
            if name != "logits_v/b":       # (one element: a single draw either way)
                assert e_slabs <= 2 * e_rows, (name, e_slabs, e_rows)
    assert not bc.SIZE_FACTOR


@pytest.mark.parametrize("head,num_actions", bc.WIDE)
def test_the_wide_heads_cases(head, num_actions):
    import image_limit_cases as ic
    for bsz in bc.WIDE_SIZES:
        xk, x, a, y = bc.wide_rows(head, num_actions, bsz)
        assert xk.shape == (bsz, 84, 84, 4) and a.shape == (bsz, num_actions) and y.shape == (bsz,)
        assert np.array_equal(x, xk.astype(np.float32) / np.float32(128.0) - np.float32(1.0))
    # 66 roles (A + 2; 2A + 2 columns under CONTINUOUS_INPUT, 66 as well) dealt over 14 role blocks, each looping three and
    # five times over the batch
    roles = (2 * num_actions if head == "cont" else num_actions) + 2
    assert roles == 66 and [bc.bwd_path(b).wide_w_passes for b in bc.WIDE_SIZES] == [3, 5]
    case = bc.wide_case(head, num_actions, 257)
    zeros = ic.zero_tensors(head, num_actions)
    for name in case.tensors:
        if name in zeros:
            assert not np.any(case.g[name]), name
        else:
            # (1e-3: the continuous head's dz carries 1 / (X^2 + Y^2), and the value cost's conv bias gradients cancel to a
            # tenth of their terms; both have an e32 of 1e-5)
            assert np.any(case.g[name]) and case.e32[name] > 0 and c.FLOOR <= case.bound(name) < 1e-3, (name, case.e32[name])
