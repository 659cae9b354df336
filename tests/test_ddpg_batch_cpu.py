"""The cases of tests/test_gpu_ddpg_batch.py (tests/ddpg_batch_cases.py builds them for both files) on the oracles alone: every
condition that makes a passing GPU test mean something, none of which needs a GPU.

  * THREADS, PER_THREADS and MAX_B are the source's, read from its text with the loops that stride by them, and SIZES holds both
    sides of each stride and the limit.
  * Every case finds its rows within the cap of its rule.
  * No compared tensor is all zero, every e32 is positive, the float32 runs stay float32.
  * wgrad_element's serial order, restated in numpy float32, stays at or below half of the bound every gradient is held to; where
    it would not with the BLAS oracle's e32, the case takes the restatement's (and the test prints which, with both values).
  * A sum that leaves out the last row, or the first row past a stride (448, 1024), moves every gradient of both nets by more
    than two bounds.
  * The rings of the prioritised draws give duplicates at every drawn size, the heavy-tailed one names slot 700 in more than
    90 % of its rows; the uniform draw's slots are distinct."""
import os
import re

import numpy as np
import pytest

import closeness as c
import ddpg_actors_oracle as do
import ddpg_batch_cases as bc
import ddpg_oracle as o
import per_oracle as per

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ga3c_amd", "csrc")
ROW_IDS = ["S%d-A%d-B%d-%s" % (S, A, B, form) for S, A, B in bc.ROW_CASES for form in bc.FORMS]
ROW_PARAMS = [(S, A, B, form) for S, A, B in bc.ROW_CASES for form in bc.FORMS]


def _row_case(S, A, B, form):
    """(64, 32) without the serial restatement, which test_gpu_ddpg_batch.py runs for it: this file's share of the suite's time."""
    return bc.row_case(S, A, B, form, (S, A) != bc.LARGE)


def test_the_sizes_sit_on_both_sides_of_the_strides_the_source_has():
    with open(os.path.join(CSRC, "ga3c_ddpg.hip")) as fh:
        src = fh.read()

    def const(name):
        return int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))
    assert (const("THREADS"), const("PER_THREADS"), const("MAX_B")) == (bc.THREADS, bc.PER_THREADS, bc.MAX_B) == (448, 1024, 4096)
    assert const("ACT_THREADS") == 256
    # the loops that take a second trip past a thread count, as the source writes them
    assert re.search(r"for \(int i = threadIdx\.x; i < B; i \+= THREADS\) ysum \+= y\[i\];", src)
    assert len(re.findall(r"for \(int i = t; i < B; i \+= THREADS\)", src)) == 2              # ddpg_popart_kernel: the sums, yn
    assert len(re.findall(r"for \(int k = t; k < B; k \+= PER_THREADS\)", src)) == 2           # per_sample_kernel: draws, weights
    assert len(re.findall(r"for \(int i = t; i < B; i \+= PER_THREADS\)", src)) == 2           # per_update_kernel: sl[], the rows
    assert re.search(r"__shared__ int32_t sl\[MAX_B\];", src) and re.search(r"for \(int j = i \+ 1; j < B; \+\+j\)", src)
    assert len(re.findall(r"for \(int r = 0; r < B; \+\+r\)", src)) == 5     # wgrad_element's three, q_stats, the soft step's logp
    assert re.search(r"check_dims\(\*cfg, MAX_S, MAX_A, MAX_B\)", src)
    for stride in (bc.THREADS, bc.PER_THREADS):
        assert stride in bc.SIZES and stride + 1 in bc.SIZES
    assert max(bc.SIZES) == bc.MAX_B and bc.CAPACITY == 2 * bc.MAX_B
    assert all(B in bc.SIZES for B in bc.STEP_SIZES + bc.OPTION_SIZES + bc.PER_SIZES)
    assert {bc.THREADS + 1, bc.MAX_B} <= set(bc.STEP_SIZES) & set(bc.OPTION_SIZES)
    assert {bc.PER_THREADS, bc.PER_THREADS + 1, bc.MAX_B} == set(bc.PER_SIZES) == set(B for d in bc.DRAWS.values() for B, _ in d)
    assert per.CHUNK == 1024 and bc.ring("near")[0] > bc.MAX_B and bc.ring("heavy-wide")[0] > bc.MAX_B


@pytest.mark.parametrize("S,A,B,form", ROW_PARAMS, ids=ROW_IDS)
def test_rows_tensors_and_the_serial_sum(S, A, B, form):
    case = _row_case(S, A, B, form)
    print("rows: settled in %d round(s)" % case.rounds)
    assert case.rounds <= 20 and all(len(t) == B for t in case.batch)
    assert case.batch[3].any() and not case.batch[3].all()                 # done rows mixed in
    for name, want in case.want.items():
        assert np.any(want), name
        assert np.asarray(case.w32[name]).dtype == np.float32, name
        assert case.blas[name] > 0.0 and case.e32[name] >= case.blas[name], name
    for name in ("y", "qt", "q"):
        assert np.asarray(case.out32[name]).dtype == np.float32 and np.any(case.out[name]), name
    # the serial sum: every weight and bias gradient of both nets
    if (S, A) == bc.LARGE:
        return
    assert set(case.serial) == set(k for k in o.TRAINABLE if k != o.DEAD)
    for k, (err, ratio) in case.serial.items():
        held = err / case.bound("grad " + k)
        print("S=%d A=%d B=%d %-6s %-20s serial %.3e  BLAS e32 %.3e  serial / bound(BLAS) %.2f  serial / bound held %.2f%s"
              % (S, A, B, form, k, err, case.blas["grad " + k], ratio, held, "  <- e32 restated" if k in case.restated else ""))
        assert held <= 0.5, (k, held)
        assert (k in case.restated) == (ratio > 0.5)


@pytest.mark.parametrize("S,A,B,form", ROW_PARAMS, ids=ROW_IDS)
def test_a_sum_short_of_one_row_moves_every_gradient_by_more_than_two_bounds(S, A, B, form):
    """What wgrad_element would leave with `r < B - 1`, or with row 448 / 1024 skipped: the gradient less that row's term (in the
    paired form this is the batch of B - 1 rows with its sums rescaled by (B - 1) / B)."""
    case = _row_case(S, A, B, form)
    src = case.sources()
    least = {}
    for row in (B - 1,) + tuple(r for r in bc.STRIDE_ROWS if r < B - 1):
        for k, s in src.items():
            want = case.want["grad " + k]
            moved = float(np.max(np.abs(bc.row_term(s, row)))) / float(np.max(np.abs(want)))
            ratio = moved / case.bound("grad " + k)
            if row not in least or ratio < least[row][0]:
                least[row] = (ratio, k)
    for row, (ratio, k) in least.items():
        print("S=%d A=%d B=%d %s: without row %d the least-moved gradient is %s, by %.1f bounds" % (S, A, B, form, row, k, ratio))
        assert ratio > 2.0, (row, k, ratio)


def test_the_sources_are_the_oracles_gradients():
    """serial_sum in float64 over the restated sources is the oracle's gradient: the restatement sums what the oracle sums."""
    case = bc.row_case(7, 3, 449, "fork")
    for k, s in case.sources().items():
        assert c.rel_err(bc.serial_sum(*s), case.want["grad " + k]) < 1e-12, k


@pytest.mark.parametrize("B", bc.STEP_SIZES)
@pytest.mark.parametrize("way", list(bc.STEP_WAYS))
def test_the_step_cases_find_their_rows_and_move_the_weights(way, B):
    case = bc.step_case(B, way)
    print("steps B=%d %s: rounds %s" % (B, way, case.rounds))
    assert len(case.batches) == 2 and all(r <= 20 for r in case.rounds)
    moved = max(float(np.max(np.abs(case.st["online"][k] - case.online[k]))) for k in o.TRAINABLE if k != o.DEAD)
    assert moved > 10 * 1e-5 and case.st["step"] == 2                      # steps that WTOL = 1e-5 can see


@pytest.mark.parametrize("B", bc.OPTION_SIZES)
def test_the_option_cases_find_their_rows(B):
    import popart_oracle as po
    online, target, batch, noise, kw = bc.popart_case(B)
    assert all(len(t) == B for t in batch) and np.all(batch[2] < -99.9) and np.all(batch[2] > -100.1)
    s1, s2 = po.kernel_sums(batch[2])
    assert abs(s1 - float(np.sum(batch[2], dtype=np.float64))) <= 1e-9 * abs(s1)
    first = po.kernel_sums(batch[2][:bc.THREADS])                          # a sum that stops after its first trip ...
    mu1, _ = po.update_mixed(bc.POPART_MU, bc.POPART_NU, batch[2], bc.POPART_BETA)
    short = np.float32((1 - bc.POPART_BETA) * bc.POPART_MU + bc.POPART_BETA * first[0] / B)
    assert abs(float(short) - float(mu1)) > 100 * np.spacing(np.abs(mu1))  # ... is far outside one spacing of mu'
    online, target, batch, noise, tried = bc.twin_case(B)
    print("twin B=%d: %d candidates tried" % (B, tried))
    assert all(len(t) == B for t in batch) and tried <= 4 * B
    import td3_oracle as t3
    eps = t3.smoothing_noise(bc.TWIN_SEED, 1, B, bc.SHAPE[1], bc.TWIN["sigma"], bc.TWIN["noise_clip"])
    at_clip = float(np.mean(np.abs(eps) == np.float32(bc.TWIN["noise_clip"])))
    assert 0.5 < at_clip < 0.95 and len(np.unique(eps)) > 0.04 * eps.size  # the clip applies to most draws, not to all
    online, target, batch, noise, rounds = bc.dist_case(B)
    print("dist B=%d: %d round(s)" % (B, rounds))
    assert all(len(t) == B for t in batch) and rounds <= 20
    online, target, batch, tried = bc.soft_case(B)
    print("soft B=%d: %d candidates tried" % (B, tried))
    assert all(len(t) == B for t in batch) and tried <= 4 * B


def test_the_rings_give_duplicates_and_the_heavy_tail_names_one_slot():
    for kind, draws in bc.DRAWS.items():
        size, pa, top = bc.ring(kind)
        assert pa.size == size and np.all(pa > 0) and float(pa.max()) <= top
        for B, number in draws:
            slots, total, clamped = bc.draw(kind, B, number)
            dup = B - len(set(slots.tolist()))
            share = float(np.mean(slots == bc.HEAVY_SLOT))
            print("ring %s B=%d: %d duplicates, %d clamped, slot %d in %.1f %% of the rows" % (kind, B, dup, clamped, bc.HEAVY_SLOT, 100 * share))
            assert slots.min() >= 0 and slots.max() < size and np.all(np.diff(slots) >= 0)
            if kind == "tail":                                              # only the last row holds the largest weight
                w = per.weights(pa, size, slots, total, 0.4)
                assert np.flatnonzero(w == 1.0).tolist() == [B - 1] and B == bc.PER_THREADS + 1
                assert slots[B - 1] >= size - bc.TAIL > slots[B - 2] and float(np.sort(w)[-2]) < 0.9
            if kind == "million":
                assert dup == 0 and slots.max() > size - 2 * size // B      # the last stratum lies in the last chunks
            elif kind != "tail":
                assert dup >= 1
            if kind == "heavy":
                assert share > 0.9
            w = per.weights(pa, size, slots, total, 0.4)
            assert w.max() == 1.0 and len(np.unique(w)) > (1 if kind == "heavy" else B // 2)
    for kind, B in bc.UPDATES:
        size, pa, _ = bc.ring(kind)
        assert size > B                                                     # train_prioritized wants MORE rows than a batch
        slots = bc.draw(kind, B, 0)[0]
        named = np.flatnonzero(slots == bc.HEAVY_SLOT)
        assert named.size > 0.9 * B and named[-1] - named[0] > bc.PER_THREADS * (B > bc.PER_THREADS + 1)
        # the rows that name it lie on both sides of the scan's first 1024 entries, and other slots follow the last of them
        assert named[-1] < B - 1


def test_the_weighted_case_finds_its_ring():
    pa, slots, w, noise, online, target, rows = bc.weighted_case()
    assert slots.size == bc.WEIGHTED["B"] == bc.PER_THREADS + 1 and len(rows[2]) == bc.WEIGHTED["n"] > slots.size
    assert len(np.unique(w)) > slots.size // 2 and w.max() == 1.0 and slots.size - len(set(slots.tolist())) >= 1


def test_the_uniform_draws_slots_are_distinct_and_fill_the_grid():
    for B in bc.ACTORS_SIZES:
        slots = do.uniform_slots(bc.DRAW_SEED, 0, bc.ACTORS_PREFILL, B)
        assert len(set(slots.tolist())) == B and slots.min() >= 0 and slots.max() < bc.ACTORS_PREFILL
        assert (B + 255) // 256 > 4 and B % 256 in (0, 1)                  # full blocks, and a block with one thread at work
    assert bc.ACTORS_PREFILL > max(bc.ACTORS_SIZES) and bc.ACTORS_PREFILL + bc.ACTORS_N <= bc.CAPACITY
