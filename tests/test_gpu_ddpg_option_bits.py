"""-m gpu: the DDPG handle's options (distributional critic, PopArt, soft actor-critic, and every create and destroy of them
and of the twin on one handle) still give the bits they gave before their variables came from one table, their arenas from one
re-lay (ga3c_amd/csrc/ga3c_ddpg_vars.hpp) and the soft step from the twin's enqueue.

The pattern, the helpers and the recorder's import check are tests/test_gpu_ddpg_parent_bits.py's, which has the plain, twin,
prioritised, n-step and actor paths.  tests/golden/ddpg_option_bits_parent.json holds SHA-256 digests of raw bytes, recorded on
an MI355X from a build of the PARENT commit of the change (an export of it, built with its own Makefile):

    python tests/test_gpu_ddpg_option_bits.py --tree <built checkout of the parent commit> --commit <its hash> \
        --record tests/golden/ddpg_option_bits_parent.json

The recording runs every case twice and leaves out a case whose two runs differ (it names them).  The test never writes the
fixture.

What a case digests:
  names       the table's variable names and their target copies' names, in order
  arena0..4   every variable of the handle's table, in table order, from ga3c_ddpg_get_param: value, target, the two slots and
              the gradient
  fetch:NAME  every name ga3c_ddpg_fetch accepts on the handle: the 24 core rows ("do" is [B, 2A] on a soft handle), the twin's
              twelve, d_* of a distributional critic, yn of PopArt, s_* of the soft actor-critic, per_w / per_td with priorities
  dist_info, popart_info, soft_info   where the handle has the option
Cases, at (S, A) = (7, 3), B = 17 (a second tile with one valid row), a ring of 48 rows (rows as test_gpu_ddpg._candidates makes
them, a given noise vector):
  dist       51 atoms on [-2, 1], three train_replay steps, with and without USE_GRAD_CLIP; one with 2 atoms
  popart     beta 0.1, three steps; one with four train_prioritized steps
  soft       on a twin at delay 2, four steps (two policy steps), with and without clipping; one at delay 1; one with device
             actors at (3, 1), the environment's shape (N = 5, 2 x 20 actor steps, training on, batch 16, 2 updates)
  lifecycle  through the C ABI on one handle (paired loss, RMSProp critic), two training steps before the first stage and after
             every stage, digests after every stage and after its steps: twin_create, soft_create, soft_destroy, twin_destroy,
             popart_create, popart_destroy, dist_create, dist_destroy, twin_create.  The trainable variables a create adds or
             reshapes (bar log_alpha) get seeded values in the value and the target arena before the stage's steps.

The lifecycle also checks, with no fixture, what no other test does in all five arenas: across every create and destroy a
variable of the same name and shape keeps its bits in arenas 0 to 4, a new or reshaped one holds the rule's constant in each
(a moving variance and nu 1 in arenas 0 and 1, log_alpha its given value there, a critic's trainable variable 1 in arena 2
under RMSProp, everything else 0), and ga3c_ddpg_param_info's `trainable` counts 20 / 30 / 31 / 20 variables of 26 / 38 / 39 / 28.
"""
import json
import os
import sys

import numpy as np
import pytest

from test_gpu_ddpg_parent_bits import RING_ROWS, TIME_LIMIT, TWIN_CFG, _make, _sha, _widths

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ddpg_option_bits_parent.json")
S, A, B = 7, 3, 17
SOFT_FETCH = dict(s_eps2="A", s_a2="A", s_logp2=1, s_vt=1, s_mu="A", s_ls="A", s_eps="A", s_u="A", s_logp=1, s_q1=1, s_q2=1)
DIST_CFG = dict(DDPG_CRITIC_LOSS="paired", DDPG_DISTRIBUTIONAL=True, DDPG_V_MIN=-2.0, DDPG_V_MAX=1.0)
POP_CFG = dict(DDPG_CRITIC_LOSS="paired", DDPG_POPART=True, DDPG_POPART_BETA=0.1)
SOFT_CFG = dict(TWIN_CFG, DDPG_SOFT=True)
LOG_ALPHA = np.float32(-1.6)
STAGES = [("twin_create", (2, 0.2, 0.5, 11)), ("soft_create", (float(LOG_ALPHA), 1.0, -3.0, -20.0, 2.0, 7)), ("soft_destroy", ()),
          ("twin_destroy", ()), ("popart_create", (0.1, 1e-4, 1e6)), ("popart_destroy", ()), ("dist_create", (51, -2.0, 1.0)),
          ("dist_destroy", ()), ("twin_create", (2, 0.2, 0.5, 12))]
# (variables, trainable ones) of the table after each stage
STAGE_COUNTS = [(38, 30), (39, 31), (38, 30), (26, 20), (28, 20), (26, 20), (26, 20), (26, 20), (38, 30)]


def _options(net):
    """What the handle carries, asked of the handle: (twin, atoms, popart, soft)."""
    names = net.get_variables_names()
    return ("critic2_fc1/W:0" in names, net.dist_info()[0], "critic_popart/mu:0" in names, "actor_soft/log_alpha:0" in names)


def _handle_digests(net, rows):
    """The table's names, its variables in arenas 0 to 4, every fetch name valid on the handle after a step of `rows` rows, and
    the options' info."""
    twin, atoms, pop, soft = _options(net)
    s, a = net.S, net.num_actions
    names = [n[:-2] for n in net.get_variables_names()]
    d = {"names": _sha(np.frombuffer("\n".join(names + net.get_target_names()).encode(), np.uint8))}
    for w in range(5):
        d["arena%d" % w] = _sha(*[net.get_variable_value(n, w) for n in names])
    plain, twelve = _widths(s, a)
    widths = dict(plain, do=2 * a if soft else a)
    if twin:
        widths.update(twelve)
    if atoms > 1:
        widths.update(d_pt=atoms, d_m=atoms, d_p=atoms, d_dz=atoms, d_ce=1)
        d["dist_info"] = _sha(np.float64(net.dist_info()))
    if pop:
        widths["yn"] = 1
        d["popart_info"] = _sha(np.float64(net.popart_info()))
    if soft:
        widths.update({k: a if v == "A" else v for k, v in SOFT_FETCH.items()})
        d["soft_info"] = _sha(np.float64(net.soft_info()))
    for name, width in widths.items():
        d["fetch:" + name] = _sha(net.fetch(name, width * rows))
    if net.prioritized:
        pa, top = net.priorities()
        d["pa"], d["max_pa"] = _sha(pa), _sha(np.float32(top))
        d["fetch:per_w"], d["fetch:per_td"] = _sha(net.fetch("per_w", rows)), _sha(net.fetch("per_td", rows))
    return d


def _steps_case(seed, steps, cfg):
    net, rng, noise = _make(S, A, seed, **cfg)
    try:
        slots = []
        for _ in range(steps):
            if net.prioritized:
                net.train_prioritized(B, noise=noise)
                slots.append(net.last_slots.copy())
            else:
                net.train_replay(rng.permutation(RING_ROWS)[:B].astype(np.int32), noise=noise)
        assert net.get_global_step() == steps
        d = _handle_digests(net, B)
        if slots:
            d["slots"] = _sha(*slots)
        return {"steps": d}
    finally:
        net.close()


def _soft_actors_case():
    n, batch = 5, 16
    net, rng, _ = _make(3, 1, 9005, max_batch=batch, capacity=1024, rows=0, **SOFT_CFG)
    try:
        net.actors_create(n, seed=77 + n, updates=2, batch=batch, draw_seed=4242)
        elapsed = np.zeros(n, np.int32)             # episodes that end inside the run, on different steps
        for i in range(n):
            if i % 3 != 2:
                elapsed[i] = TIME_LIMIT - 3 - (7 * i) % 31
        net.actors_set("elapsed", elapsed)
        stats, episodes = [], []
        for _ in range(2):
            stats += net.actors_run(20, train=True)
            episodes += net.actors_episodes()
        assert stats[1] > 0 and stats[5] > 0 and episodes, (stats, len(episodes))     # it trained, and episodes ended
        d = _handle_digests(net, batch)
        for f in ("phys", "elapsed", "draws", "obs", "action", "reward", "done", "slots"):
            d["actor:" + f] = _sha(net.actors_get(f))
        size, total = net.replay_size()
        d["ring"] = _sha(np.int64([size, total]), *[np.concatenate([np.ravel(t) for t in net.replay_get(k)]) for k in range(size)])
        d["episodes"] = _sha(np.float64([e[0] for e in episodes]), np.int64([e[1] for e in episodes]))
        d["stats"] = _sha(np.int64(stats))
        return {"steps": d}
    finally:
        net.close()


def _rule(name, trainable, arena, critic_adam):
    """The value a new or reshaped variable starts from in `arena`."""
    if name.endswith("/moving_variance") or name == "critic_popart/nu":
        return np.float32(1.0 if arena <= 1 else 0.0)
    if name == "actor_soft/log_alpha":
        return LOG_ALPHA if arena <= 1 else np.float32(0.0)
    if name.startswith("critic") and trainable and arena == 2 and not critic_adam:
        return np.float32(1.0)
    return np.float32(0.0)


def _snapshot(net):
    """{variable: (trainable, [its value in arenas 0 to 4])}"""
    return {n[:-2]: (net._param_info(n[:-2])[2], [net.get_variable_value(n[:-2], w) for w in range(5)])
            for n in net.get_variables_names()}


def _lifecycle():
    """-> (digests by stage, what the arena rule found wrong: empty when it holds)"""
    net, rng, noise = _make(S, A, 9100, DDPG_CRITIC_LOSS="paired", RMSPROP=True)
    out, wrong = {}, []

    def train():
        for _ in range(2):
            net.train_replay(rng.permutation(RING_ROWS)[:B].astype(np.int32), noise=noise)

    try:
        train()
        for i, ((op, args), counts) in enumerate(zip(STAGES, STAGE_COUNTS)):
            before = _snapshot(net)
            net._call(op, *args)
            after = _snapshot(net)
            if (len(after), sum(t for t, _ in after.values())) != counts:
                wrong.append((i, op, "table", len(after), sum(t for t, _ in after.values())))
            fresh = []
            for name, (trainable, values) in after.items():
                kept = name in before and before[name][1][0].shape == values[0].shape
                if not kept:
                    fresh.append(name)
                for w in range(5):
                    if kept and before[name][1][w].tobytes() != values[w].tobytes():
                        wrong.append((i, op, name, w, "moved"))
                    if not kept and not np.all(values[w] == _rule(name, trainable, w, False)):
                        wrong.append((i, op, name, w, "not the rule's constant"))
            out["%d_%s" % (i, op)] = _handle_digests(net, B)
            for name in fresh:                      # weights to train on, where the rule left zeros
                if after[name][0] and name != "actor_soft/log_alpha":
                    v = rng.normal(0.0, 0.05, after[name][1][0].shape).astype(np.float32)
                    net.set_variable_value(name, v, 0)
                    net.set_variable_value(name, v, 1)
            train()
            out["%d_%s_steps" % (i, op)] = _handle_digests(net, B)
        return out, wrong
    finally:
        net.close()


CASES = {"dist_atoms51_noclip": (_steps_case, (9001, 3, dict(DIST_CFG, DDPG_ATOMS=51, USE_GRAD_CLIP=False))),
         "dist_atoms51_clip": (_steps_case, (9001, 3, dict(DIST_CFG, DDPG_ATOMS=51, USE_GRAD_CLIP=True))),
         "dist_atoms2": (_steps_case, (9002, 3, dict(DIST_CFG, DDPG_ATOMS=2))),
         "popart": (_steps_case, (9003, 3, POP_CFG)),
         "popart_per": (_steps_case, (9003, 4, dict(POP_CFG, PRIORITIZED_REPLAY=True))),
         "soft_delay2_noclip": (_steps_case, (9004, 4, dict(SOFT_CFG, USE_GRAD_CLIP=False))),
         "soft_delay2_clip": (_steps_case, (9004, 4, dict(SOFT_CFG, USE_GRAD_CLIP=True))),
         "soft_delay1": (_steps_case, (9004, 4, dict(SOFT_CFG, DDPG_POLICY_DELAY=1))),
         "soft_actors_N5": (_soft_actors_case, ()),
         "lifecycle": (lambda: _lifecycle()[0], ())}


def _run(case):
    fn, args = CASES[case]
    return fn(*args)


@pytest.fixture(scope="module")
def parent_bits():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def lifecycle():
    return _lifecycle()


def _same_as_parent(case, got, want):
    assert sorted(got) == sorted(want)
    differ = {part: sorted(k for k in set(got[part]) | set(want[part]) if got[part].get(k) != want[part].get(k)) for part in got}
    print(case, {p: (len(got[p]), "digests") for p in got})
    assert not any(differ.values()), differ


def test_the_parent_agreed_with_itself_on_every_case(parent_bits):
    assert parent_bits["left_out"] == [] and sorted(parent_bits["digests"]) == sorted(CASES)


@pytest.mark.parametrize("case", sorted(c for c in CASES if c != "lifecycle"))
def test_option_bits_are_the_parents(parent_bits, case):
    if case not in parent_bits["digests"]:
        pytest.fail("%s is not in the fixture" % case)
    _same_as_parent(case, _run(case), parent_bits["digests"][case])


def test_lifecycle_bits_are_the_parents(parent_bits, lifecycle):
    if "lifecycle" not in parent_bits["digests"]:
        pytest.fail("lifecycle is not in the fixture")
    _same_as_parent("lifecycle", lifecycle[0], parent_bits["digests"]["lifecycle"])


def test_every_create_and_destroy_keeps_or_starts_every_variable_in_all_five_arenas(lifecycle):
    assert len(lifecycle[0]) == 2 * len(STAGES)
    assert lifecycle[1] == []


def _record(tree, out, commit):
    """Digests of the build in `tree` (a built checkout of the parent commit) -> the fixture."""
    tree = os.path.abspath(tree)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert os.path.realpath(tree) != os.path.realpath(here), "--tree must be a checkout of the parent, not this tree"
    sys.path[:0] = [tree]
    import ga3c_amd
    import _native
    import NetworkDDPG
    for mod, path in ((ga3c_amd, ga3c_amd.__file__), (_native, _native.__file__), (NetworkDDPG, NetworkDDPG.__file__),
                      (_native, _native.HIP_LIB)):
        assert os.path.realpath(path).startswith(os.path.realpath(tree) + os.sep), (mod, path)
    assert os.path.exists(_native.HIP_LIB), "the parent checkout is not built"
    digests, unstable = {}, []
    for case in sorted(CASES):
        first, second = _run(case), _run(case)
        if first != second:
            unstable.append(case)
            print("LEFT OUT %s: the parent's own two runs differ" % case, flush=True)
            continue
        digests[case] = first
        print("recorded %s" % case, flush=True)
    with open(out, "w") as f:
        json.dump({"what": "sha256 of raw bytes of each case of tests/test_gpu_ddpg_option_bits.py",
                   "recorded_from": "a build of the parent commit %s on an MI355X (gfx950)" % commit,
                   "left_out": unstable, "digests": digests}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("recorded %d cases from %s, left out %d: %s" % (len(digests), tree, len(unstable), unstable))


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", required=True)
    ap.add_argument("--record", required=True)
    ap.add_argument("--commit", required=True, help="the parent commit that --tree is a checkout of")
    args = ap.parse_args()
    _record(args.tree, args.record, args.commit)
