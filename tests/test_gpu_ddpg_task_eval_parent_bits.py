"""-m gpu: the DDPG device actors' step and the evaluation episode, folded from eight kernels into four (one ddpg_actors_step_kernel
and one ddpg_actors_nstep_kernel that always take the task from their arguments, one ddpg_eval_kernel<Env, Policy> for the
deterministic and the soft actor), still give the bits the eight gave.

The pattern and the helpers are tests/test_gpu_ddpg_parent_bits.py's, which with tests/test_gpu_ddpg_option_bits.py already has
the actors' step without a task (N = 5 and 257, n = 1, 3 and 16, twin, priorities, the soft handle).  This file has what those
leave: the step under a task that is not the fork's, and every evaluation.  tests/golden/ddpg_task_eval_bits_parent.json holds
SHA-256 digests of raw bytes, recorded on an MI355X from a build of the PARENT commit of the change (an export of it, built with
its own Makefile):

    python tests/test_gpu_ddpg_task_eval_parent_bits.py --tree <built checkout of the parent commit> --commit <its hash> \
        --record tests/golden/ddpg_task_eval_bits_parent.json

The recording imports the package and the library from --tree, never from this tree, runs every case twice and leaves out a
case whose two runs differ (it names them).  The test below never writes the fixture, and fails for a case that is not in it.

All cases at (S, A) = (3, 1), the environment's.  GYM: clip, truncate, reset_observation, reward scale 1 and offset 0.
  eval         a plain handle after two train steps (the target arena is no longer the value arena); n in 1, 17, 33: one row of
               a 16-row tile, a second tile with one row, three tiles; eval_run(200) on the value arena, then
               eval_run(3, target=True); after each run the totals, phys and the four trace fields
  eval_task    n = 17 under GYM, the same two runs
  eval_soft    a soft handle on a twin, n = 17, without a task and under GYM; eval_run(6), then eval_run(200)
  actors_task  test_gpu_ddpg_parent_bits._actors_case's recipe under GYM: N in 5, 257 (one partial block, one thread alone in a
               second block of 256), DDPG_NSTEP 1 and 3, 40 actor steps over two actors_run calls with training on, batch 16,
               2 updates, episodes that end inside the run on different steps; its digests
"""
import json
import os

import numpy as np
import pytest

from test_gpu_ddpg_parent_bits import RING_ROWS, _actors_case, _main, _make, _run, _sha

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ddpg_task_eval_bits_parent.json")
S, A, B = 3, 1, 16
GYM = ('clip', 'truncate', True, 1.0, 0.0)
SOFT_CFG = dict(DDPG_CRITIC_LOSS="paired", DDPG_TWIN=True, DDPG_POLICY_DELAY=2, DDPG_TARGET_NOISE=0.2, DDPG_TARGET_NOISE_CLIP=0.5,
                DDPG_SOFT=True)
EVAL_FIELDS = ("phys", "trace_phys", "trace_obs", "trace_action", "trace_reward")


def _eval_digests(net, steps, target=False):
    total = net.eval_run(steps, target=target)
    assert np.all(np.isfinite(total)) and np.all(total < 0.0)
    return dict({"total": _sha(total)}, **{f: _sha(net.eval_get(f)) for f in EVAL_FIELDS})


def _eval_case(n, task):
    net, rng, noise = _make(S, A, 6000 + n, DDPG_CRITIC_LOSS="paired")
    try:
        for _ in range(2):
            net.train_replay(rng.permutation(RING_ROWS)[:B].astype(np.int32), noise=noise)
        if task:
            net.task_create(*task)
        net.eval_create(n, seed=6100 + n, trace=True)
        return {"value200": _eval_digests(net, 200), "target3": _eval_digests(net, 3, target=True)}
    finally:
        net.close()


def _eval_soft_case(task):
    n = 17
    net, _, _ = _make(S, A, 6200, rows=0, **SOFT_CFG)
    try:
        if task:
            net.task_create(*task)
        net.eval_create(n, seed=6300, trace=True)
        return {"value6": _eval_digests(net, 6), "value200": _eval_digests(net, 200)}
    finally:
        net.close()


CASES = {}
for _n in (1, 17, 33):
    CASES["eval_n%d" % _n] = (_eval_case, (_n, None))
CASES["eval_task_n17"] = (_eval_case, (17, GYM))
CASES["eval_soft_n17"] = (_eval_soft_case, (None,))
CASES["eval_soft_task_n17"] = (_eval_soft_case, (GYM,))
for _N in (5, 257):
    for _n in (1, 3):
        CASES["actors_task_N%d_n%d" % (_N, _n)] = (_actors_case, (_N, _n, "plain", GYM))


@pytest.fixture(scope="module")
def parent_bits():
    with open(FIXTURE) as f:
        return json.load(f)["digests"]


@pytest.mark.parametrize("case", sorted(CASES))
def test_task_and_eval_bits_are_the_parents(parent_bits, case):
    if case not in parent_bits:
        pytest.fail("%s is not in the fixture" % case)
    got, want = _run(case, CASES), parent_bits[case]
    assert sorted(got) == sorted(want)
    differ = {part: sorted(k for k in set(got[part]) | set(want[part]) if got[part].get(k) != want[part].get(k)) for part in got}
    print(case, {p: (len(got[p]), "digests") for p in got})
    assert not any(differ.values()), differ


if __name__ == "__main__":
    _main(cases=CASES, what="of each case of tests/test_gpu_ddpg_task_eval_parent_bits.py")
