"""The cases of tests/test_gpu_vector_batch.py (tests/vector_batch_cases.py builds them for both files) on the oracles alone: every
condition that makes a passing GPU test mean something, none of which needs a GPU.

  * 65536, TILE = 16, ROWS_AHEAD = 16 and the row loops of elem_grad / sum_rows / dot_rows, with their chains in double, are the
    source's, read from its text; Config's row limit for the device actors is the create limit.
  * No compared tensor is all zero, every e32 is positive, the float32 runs stay float32.
  * The kernels' chains, restated in numpy (float32 operands, a chain in double rounded once), stay at or below half of the bound
    every gradient is held to.
  * The actors' oracles at the two device-actor cases lay out exactly N x T1 = 65536 rows at the first cut.
  * On the heavy batches a sum without the heavy row, or without the whole last tile, moves every gradient of the network by more
    than two bounds at every size; on the plain batches the same figure is printed, not asserted (a lost row is not visible there).
  * The exchange of one row's term (Case._swap) gives what the oracle gives on the heavy batch."""
import os
import re

import numpy as np
import pytest

import closeness as c
import vector_batch_cases as vb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ga3c_amd", "csrc")


def _text(*path):
    with open(os.path.join(*path)) as fh:
        return fh.read()


def test_the_limit_the_tile_and_the_row_loops_are_the_sources():
    tile, mlp, dmlp = _text(CSRC, "ga3c_tile.hpp"), _text(CSRC, "ga3c_mlp.hip"), _text(CSRC, "ga3c_dmlp.hip")
    assert int(re.search(r"constexpr int TILE = (\d+);", tile).group(1)) == vb.TILE == 16
    assert int(re.search(r"constexpr int ROWS_AHEAD = (\d+);", tile).group(1)) == vb.ROWS_AHEAD == 16
    for src in (mlp, dmlp):
        assert re.search(r"check_dims\(\*cfg, MAX_S, MAX_A, %d\)" % vb.MAX_BATCH, src)
        assert re.search(r"dim3\(\(B \+ TILE - 1\) / TILE\)", src)
        assert re.search(r"const int row0 = blockIdx\.x \* TILE, nrows = min\(TILE, B - row0\);", src)
    # elem_grad: two loops over all the rows in row order, the accumulators double, one rounding at the end
    body = mlp[mlp.index("void elem_grad("):mlp.index("__global__ __launch_bounds__(THREADS) void mlp_wgrad_kernel")]
    assert len(re.findall(r"for \(int r = 0; r < B; \+\+r\)", body)) == 2
    assert re.search(r"double s\[NC\];", body) and not re.search(r"\bfmaf\(|g\[c\] \+=", body)
    assert re.search(r"g\[c\] = \(float\)s\[c\];", body)
    # sum_rows / dot_rows: blocks of ROWS_AHEAD rows, then the tail to B, the accumulator double in both
    rows = tile[tile.index("float sum_rows("):tile.index("void loss_sums(")]
    assert len(re.findall(r"for \(; r \+ ROWS_AHEAD <= B; r \+= ROWS_AHEAD\)", rows)) == 2
    assert len(re.findall(r"for \(; r < B; \+\+r\)", rows)) == 2
    assert len(re.findall(r"double g = 0\.0;", rows)) == 2 and len(re.findall(r"return \(float\)g;", rows)) == 2
    assert not re.search(r"float g\b|\bfmaf\(", rows)
    assert re.search(r"losses\[threadIdx\.x\] = sum_rows\(lossrow \+ threadIdx\.x, 3, B\);", tile)
    assert re.search(r"\bsum_rows\([^;]*, B\);", dmlp) and re.search(r"\bdot_rows\([^;]*, B\);", dmlp)
    # the sizes: past what the older files run, both tails, the limit short by one and full
    assert vb.SIZES == [1025, 4099, 16384, 65535, 65536] and max(vb.SIZES) == vb.MAX_BATCH
    assert 4099 % vb.TILE == 4099 % vb.ROWS_AHEAD == 3 and 65535 % vb.TILE == 15
    assert set(vb.LARGE_SIZES) <= set(vb.SIZES) and set(vb.STEP_SIZES) <= set(vb.SIZES)
    assert [vb.last_tile(B) for B in (16, 17, 65535, 65536)] == [0, 16, 65520, 65520]


def test_configs_row_limit_is_the_create_limit():
    cfg = _text(ROOT, "ga3c_amd", "Config.py")
    assert int(re.search(r"rows = n \* \(Config\.TIME_MAX \+ 1\)\n\s+if rows > (\d+):", cfg).group(1)) == vb.MAX_BATCH
    actors = _text(CSRC, "ga3c_actors.hpp")
    assert re.search(r"if \(\(int64_t\)n \* T1 > m->max_batch\)", actors)


def test_the_shapes_are_the_older_files():
    import test_gpu_dmlp as td
    assert vb.NETS["dmlp-eight"][1:] == td.EIGHT[0] and vb.NETS["dmlp-fork"][1:] == td.SHAPES[0]
    assert vb.NETS["dmlp-chained"][1:] == td.SHAPES[1]
    assert all(vb.DMLP_HEADS[h] == td.HEADS[h] for h in vb.DMLP_HEADS)
    assert max(td.SIZES) < min(vb.SIZES)
    assert len(vb.CASES) == 5 + 2 + 2 * (5 + 5 + 2)


@pytest.mark.parametrize("net_id,head,B", vb.CASES, ids=vb.CASE_IDS)
def test_tensors_the_serial_sum_and_a_sum_short_of_rows(net_id, head, B):
    cs = vb.case(net_id, head, B)
    n = cs.net
    assert cs.x.shape == (B, n.S) and cs.x.dtype == np.float32
    for kind in vb.KINDS:
        want, w32 = cs.want[kind], cs.w32[kind]
        for k in n.acts + n.deltas + n.grads:
            assert np.any(want[k]), (kind, k)
            assert np.asarray(w32[k]).dtype == np.float32 and np.asarray(want[k]).dtype == np.float64, (kind, k)
        for k in n.deltas + n.grads:
            assert cs.e32[kind][k] > 0.0, (kind, k)
        assert set(cs.serial[kind]) == set(n.grads)
        for k, (err, held) in cs.serial[kind].items():
            print("%s %s B=%d %-5s %-18s restated chain %.3e  e32 %.3e  restated / bound %.3f" % (net_id, head, B, kind, k, err,
                                                                                                cs.e32[kind][k], held))
            assert held <= 0.5, (kind, k, held)
    # a sum short of the heavy row, or of the last tile
    tile = np.arange(vb.last_tile(B), B)
    for kind in vb.KINDS:
        for what, rows in (("row", np.array([B - 1 if kind == "plain" else vb.heavy_row(kind, B)])), ("last tile", tile)):
            term = cs.rows_term(kind, rows)
            ratio, k = min((float(np.max(np.abs(term[k]))) / float(np.max(np.abs(cs.want[kind][k]))) / cs.bound(kind, k), k)
                           for k in n.grads)
            print("%s %s B=%d %-5s: without the %s the least-moved gradient is %s, by %.2f bounds" % (net_id, head, B, kind, what, k, ratio))
            assert kind == "plain" or ratio > 2.0, (kind, what, k, ratio)


@pytest.mark.parametrize("net_id,head", [("mlp-3-1", "angle"), ("dmlp-chained", "log_softmax"), ("dmlp-fork", "plain")])
def test_the_exchanged_row_is_the_oracle_on_the_heavy_batch(net_id, head):
    """Case._swap against the oracle run on the heavy batch itself, in float64 and in float32 (where two orders of one sum differ
    by float32 rounding: held to 16 x closeness.FLOOR)."""
    cs = vb.case(net_id, head, 1025)
    n = cs.net
    for kind in ("last", "tile"):
        assert cs.y[kind][vb.heavy_row(kind, 1025)] == np.float32(vb.HEAVY) * cs.y["plain"][vb.heavy_row(kind, 1025)]
        assert int(np.sum(cs.y[kind] != cs.y["plain"])) == 1
        losses, t = n.grads_of(n.params, cs.x, cs.y[kind], cs.a)
        for k in n.deltas + n.grads:
            assert c.rel_err(cs.want[kind][k], t[k]) < 1e-12, (kind, k)
        for k in vb.LOSSES:
            assert abs(losses[k] - cs.losses[kind][k]) <= 1e-12 * abs(losses[k]), (kind, k)
        _, t32 = n.grads_of(vb.vc.f32_params(n.params), cs.x, cs.y[kind], cs.a)
        for k in n.deltas + n.grads:
            assert c.rel_err(cs.w32[kind][k], t32[k]) < 16 * c.FLOOR, (kind, k)


def test_the_serial_sum_on_the_float64_tensors_is_the_oracles_gradient():
    """The restatement sums what the oracle sums: on the oracle's float64 inputs and deltas it is the oracle's gradient."""
    for net_id, head in (("dmlp-chained", "plain"), ("dmlp-fork", "log_softmax"), ("mlp-3-1", "angle")):
        cs = vb.case(net_id, head, 1025)
        for wn, bn, x, d in cs.net.sources(cs.want["plain"]):
            g, b = vb.serial_sum(x, d)
            assert c.rel_err(g, cs.want["plain"][wn]) < 1e-12 and c.rel_err(b, cs.want["plain"][bn]) < 1e-12, (net_id, wn)


def test_the_step_cases_move_the_weights_and_the_permutation_moves_the_rows():
    perm = vb.permutation(vb.MAX_BATCH)
    assert sorted(perm.tolist()) == list(range(vb.MAX_BATCH)) and float(np.mean(perm == np.arange(vb.MAX_BATCH))) < 0.001
    assert perm[0] // vb.TILE != 0 and max(vb.SAME_ROWS) == vb.MAX_BATCH - 1 and vb.last_tile(vb.MAX_BATCH) in vb.SAME_ROWS
    for net_id, head in vb.STEP_NETS:
        n = vb.net(net_id, head)
        for B in vb.STEP_SIZES:
            ref = {k: v.copy() for k, v in n.params.items()}
            ms = {k: np.ones_like(v) for k, v in ref.items()}
            mom = {k: np.zeros_like(v) for k, v in ref.items()}
            g = n.train_step(ref, ms, mom, *vb.step_batch(net_id, head, B, 0), vb.STEP_LR)
            moved = max(float(np.max(np.abs(ref[k] - n.params[k]))) for k in n.grads)
            norms = min(float(np.sqrt(np.sum(g[k] ** 2)) / g[k].size) for k in n.grads)
            print("%s B=%d: one step moves a weight by up to %.2e; least ||g|| / n %.2e" % (net_id, B, moved, norms))
            assert moved > 10 * 1e-5 and norms > 1.5 * vb.STEP_CLIP


@pytest.mark.parametrize("game", list(vb.ACTOR_CASES))
def test_the_actors_oracles_lay_out_the_row_limit_at_the_first_cut(game):
    """N x (TIME_MAX + 1) = 65536 rows, 16 environments per thread of the 1024-thread scan; nothing is cut before step
    TIME_MAX + 1, no episode ends by itself up to it, and the forced ones (test_gpu_device_agents._forced) end on it."""
    from test_gpu_device_agents import _forced
    ora, n, time_max = vb.actors_oracle(game)
    assert n * (time_max + 1) == vb.MAX_BATCH and -(-n // 1024) == 16
    forced = _forced(n)
    p = np.full((n, 2), 0.5) if game == "cartpole" else np.zeros((n, 1), np.float32)
    for step in range(time_max + 2):
        if step == time_max + 1:
            for i in forced:
                ora.env[i].elapsed = 199
        res, batch, episodes = ora.step(p)
        if step <= time_max:
            assert batch is None and not episodes and not any(r["own_done"] for r in res), step
    assert all(len(t) == vb.MAX_BATCH for t in batch) and len(episodes) == len(forced)
    assert np.array_equal(np.flatnonzero([r["own_done"] for r in res]), forced)
