"""-m gpu: the DDPG step paths that were folded into one (one target / critic / wgrad / update kernel compiled for one or two
critics, one statement of the actor step, one enqueue on the host) still give the bits they gave before.

The other DDPG tests hold a step to f64 oracles at tolerances; a refactor can stay inside those and still reorder a sum.
tests/golden/ddpg_bits_parent.json holds SHA-256 digests of raw bytes, recorded on an MI355X from a build of the PARENT commit
of the change (an export of it, built with its own Makefile):

    python tests/test_gpu_ddpg_parent_bits.py --tree <built checkout of the parent commit> --commit <its hash> \
        --record tests/golden/ddpg_bits_parent.json

The recording imports the package and the library from --tree, never from this tree, runs every case twice and leaves out a
case whose two runs differ (it names them).  The test below never writes the fixture.

What a case digests, after its last step:
  arena0..3   every variable of the handle's table, in table order, from ga3c_ddpg_get_param
  fetch:NAME  every name ga3c_ddpg_fetch accepts on the handle (the twin's twelve, per_w / per_td, disc where they exist)
  pa, max_pa  ga3c_ddpg_priorities_get, on a handle with priorities;  nstep_disc  ga3c_ddpg_nstep_get, with n-step returns
  actor:FIELD ga3c_ddpg_actors_get's fields, ring: every slot written from ga3c_ddpg_replay_get, episodes: the records of
              ga3c_ddpg_actors_episodes, for the actor cases
Cases (rows as test_gpu_ddpg._candidates makes them, added by replay_add; a given noise vector):
  train   (S, A) in (3, 1), (7, 3); B in 1, 17, 33: one valid row of a 16-row tile, a second tile with one row, three tiles;
          three train_replay steps on a seeded permutation of slots; "fork": the fork's loss, RMSProp critic; "clipadam": paired
          loss, GRAD_CLIP, Adam critic; at B = 17 a compute at stop_after 3 and one at 4 follow
  twin    the same shapes and B, delay 2, sigma 0.2, clip 0.5, four steps (two policy steps), with and without GRAD_CLIP; one
          with sigma 0
  twinper B = 17, four train_prioritized steps
  nstep   n = 3, seeded discounts by slot (ga3c_ddpg_nstep_set), one plain and one twin step at B = 17
  actors  (3, 1); N in 5, 257: one partial block, one thread alone in a second block of 256; n in 1, 3, 16; 40 actor steps over
          two actors_run calls with training on, batch 16, 2 updates; one with the twin attached, one with priorities
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ddpg_bits_parent.json")
SHAPES = [(3, 1), (7, 3)]
SIZES = [1, 17, 33]
RING_ROWS = 48                      # rows in the ring of a train case: more than the largest batch
TIME_LIMIT = 200                    # Pendulum-v0's, device_pendulum_oracle.TIME_LIMIT
H1, H2 = 400, 300
TRAIN_CFG = {"fork": dict(DDPG_CRITIC_LOSS="fork", RMSPROP=True),
             "clipadam": dict(DDPG_CRITIC_LOSS="paired", USE_GRAD_CLIP=True, RMSPROP=False)}
TWIN_CFG = dict(DDPG_CRITIC_LOSS="paired", DDPG_TWIN=True, DDPG_POLICY_DELAY=2, DDPG_TARGET_NOISE=0.2,
                DDPG_TARGET_NOISE_CLIP=0.5)


def _widths(S, A):
    w = {"y": 1, "qt": 1, "q": 1, "dq": 1, "c_x": S, "c_a": A, "c_xh1": H1, "c_c1": H1, "c_dn1": H1, "c_dh1": H1, "c_c2": H2,
         "c_dt": H2, "a_xh1": H1, "a_a1": H1, "a_dn1": H1, "a_dh1": H1, "a_xh2": H2, "a_a2": H2, "a_dn2": H2, "a_dh2": H2,
         "a_out": A, "a_noisy": A, "g": A, "do": A}
    twin = {"qt1": 1, "qt2": 1, "q2": 1, "dq2": 1, "t_eps": A, "t_a": A, "c2_xh1": H1, "c2_c1": H1, "c2_dn1": H1, "c2_dh1": H1,
            "c2_c2": H2, "c2_dt": H2}
    return w, twin


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _handle_digests(net, B):
    """The variables in arenas 0 to 3 and every fetch name valid on the handle after a step of B rows."""
    names = [n[:-2] for n in net.get_variables_names()]
    d = {"arena%d" % w: _sha(*[net.get_variable_value(n, w) for n in names]) for w in range(4)}
    plain, twin = _widths(net.S, net.num_actions)
    for name, width in list(plain.items()) + (list(twin.items()) if net.twin else []):
        d["fetch:" + name] = _sha(net.fetch(name, width * B))
    if net.prioritized:
        pa, top = net.priorities()
        d["pa"], d["max_pa"] = _sha(pa), _sha(np.float32(top))
        d["fetch:per_w"], d["fetch:per_td"] = _sha(net.fetch("per_w", B)), _sha(net.fetch("per_td", B))
    if net.nstep > 1:
        d["nstep_disc"], d["fetch:disc"] = _sha(net.nstep_discounts()), _sha(net.fetch("disc", B))
    return d


def _make(S, A, seed, max_batch=64, capacity=64, rows=RING_ROWS, **cfg):
    """A handle with the package's seeded initial weights and `rows` seeded rows in its ring."""
    from test_gpu_ddpg import _candidates, _net
    net = _net(S, A, max_batch=max_batch, capacity=capacity, **cfg)
    rng = np.random.Generator(np.random.PCG64(seed))
    if rows:
        net.replay_add(*_candidates(S, A, rows, rng))
    return net, rng, np.linspace(-0.2, 0.3, A).astype(np.float32)


def _train_case(S, A, B, cfg):
    from test_gpu_ddpg import _candidates
    net, rng, noise = _make(S, A, 1000 + 10 * B + S, **TRAIN_CFG[cfg])
    out = {}
    try:
        for _ in range(3):
            net.train_replay(rng.permutation(RING_ROWS)[:B].astype(np.int32), noise=noise)
        out["steps"] = _handle_digests(net, B)
        if B == 17:
            s, a, r, done, s2 = _candidates(S, A, B, rng)
            for stop in (3, 4):
                q = net.compute(s, r, a, s2, done, stop, noise=noise)
                out["compute%d" % stop] = dict(_handle_digests(net, B), q_stats=_sha(np.float32(q)))
    finally:
        net.close()
    return out


def _twin_case(S, A, B, clip, sigma):
    net, rng, noise = _make(S, A, 2000 + 10 * B + S, **dict(TWIN_CFG, USE_GRAD_CLIP=clip, DDPG_TARGET_NOISE=sigma))
    try:
        for _ in range(4):
            net.train_replay(rng.permutation(RING_ROWS)[:B].astype(np.int32), noise=noise)
        assert net.get_global_step() == 4
        return {"steps": _handle_digests(net, B)}
    finally:
        net.close()


def _twinper_case():
    S, A, B = 7, 3, 17
    net, rng, noise = _make(S, A, 3000, **dict(TWIN_CFG, PRIORITIZED_REPLAY=True))
    try:
        slots = []
        for _ in range(4):
            net.train_prioritized(B, noise=noise)
            slots.append(net.last_slots.copy())
        return {"steps": dict(_handle_digests(net, B), slots=_sha(*slots))}
    finally:
        net.close()


def _nstep_case(twin):
    S, A, B = 7, 3, 17
    net, rng, noise = _make(S, A, 4000, **dict(TWIN_CFG if twin else TRAIN_CFG["clipadam"], DDPG_NSTEP=3))
    try:
        net.set_nstep_discounts(rng.uniform(0.0, 1.0, net.replay_capacity).astype(np.float32))
        net.train_replay(rng.permutation(RING_ROWS)[:B].astype(np.int32), noise=noise)
        return {"steps": _handle_digests(net, B)}
    finally:
        net.close()


def _actors_case(N, n, kind, task=None):
    """task: attached before the actors are made (tests/test_gpu_ddpg_task_eval_parent_bits.py); None here."""
    S, A, B, cap = 3, 1, 16, 1024
    cfg = dict(DDPG_CRITIC_LOSS="paired", DDPG_NSTEP=n)
    if kind == "twin":
        cfg = dict(TWIN_CFG, DDPG_NSTEP=n)
    elif kind == "per":
        cfg["PRIORITIZED_REPLAY"] = True
    net, rng, _ = _make(S, A, 5000 + N + n, max_batch=max(N, B), capacity=cap, rows=0, **cfg)
    try:
        if task:
            net.task_create(*task)
        net.actors_create(N, seed=77 + N, updates=2, batch=B, draw_seed=4242)
        elapsed = np.zeros(N, np.int32)             # episodes that end inside the run, on different steps
        for i in range(N):
            if i % 3 != 2:
                elapsed[i] = TIME_LIMIT - 3 - (7 * i) % 31
        net.actors_set("elapsed", elapsed)
        stats, episodes = [], []
        for _ in range(2):
            stats += net.actors_run(20, train=True, noise=[0.3])
            episodes += net.actors_episodes()
        assert stats[1] > 0 and stats[5] > 0 and episodes, (stats, len(episodes))     # it trained, and episodes ended
        d = _handle_digests(net, B)
        for f in ("phys", "elapsed", "draws", "obs", "action", "reward", "done", "slots"):
            d["actor:" + f] = _sha(net.actors_get(f))
        d["actor:nstep_count"] = _sha(np.int64(net.actors_get("nstep_count")))
        size, total = net.replay_size()
        d["ring"] = _sha(np.int64([size, total]), *[np.concatenate([np.ravel(t) for t in net.replay_get(k)]) for k in range(size)])
        d["episodes"] = _sha(np.float64([e[0] for e in episodes]), np.int64([e[1] for e in episodes]))
        d["stats"] = _sha(np.int64(stats))
        return {"steps": d}
    finally:
        net.close()


CASES = {}
for _S, _A in SHAPES:
    for _B in SIZES:
        for _cfg in TRAIN_CFG:
            CASES["train_S%dA%d_B%d_%s" % (_S, _A, _B, _cfg)] = (_train_case, (_S, _A, _B, _cfg))
        for _clip in (False, True):
            CASES["twin_S%dA%d_B%d_%s" % (_S, _A, _B, "clip" if _clip else "noclip")] = (_twin_case, (_S, _A, _B, _clip, 0.2))
CASES["twin_S7A3_B17_sigma0"] = (_twin_case, (7, 3, 17, False, 0.0))
CASES["twinper_S7A3_B17"] = (_twinper_case, ())
CASES["nstep_S7A3_B17_plain"] = (_nstep_case, (False,))
CASES["nstep_S7A3_B17_twin"] = (_nstep_case, (True,))
for _N in (5, 257):
    for _n in (1, 3, 16):
        CASES["actors_N%d_n%d" % (_N, _n)] = (_actors_case, (_N, _n, "plain"))
CASES["actors_N5_n3_twin"] = (_actors_case, (5, 3, "twin"))
CASES["actors_N257_n1_per"] = (_actors_case, (257, 1, "per"))


def _run(case, cases=CASES):
    fn, args = cases[case]
    return fn(*args)


@pytest.fixture(scope="module")
def parent_bits():
    with open(FIXTURE) as f:
        return json.load(f)["digests"]


@pytest.mark.parametrize("case", sorted(CASES))
def test_ddpg_bits_are_the_parents(parent_bits, case):
    if case not in parent_bits:
        pytest.fail("%s is not in the fixture" % case)
    got, want = _run(case), parent_bits[case]
    assert sorted(got) == sorted(want)
    differ = {part: sorted(k for k in set(got[part]) | set(want[part]) if got[part].get(k) != want[part].get(k)) for part in got}
    print(case, {p: (len(got[p]), "digests") for p in got})
    assert not any(differ.values()), differ


def _record(tree, out, commit, cases=CASES, what="after the last step of each case of tests/test_gpu_ddpg_parent_bits.py"):
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
    for case in sorted(cases):
        first, second = _run(case, cases), _run(case, cases)
        if first != second:
            unstable.append(case)
            print("LEFT OUT %s: the parent's own two runs differ" % case, flush=True)
            continue
        digests[case] = first
        print("recorded %s" % case, flush=True)
    with open(out, "w") as f:
        json.dump({"what": "sha256 of raw bytes " + what,
                   "recorded_from": "a build of the parent commit %s on an MI355X (gfx950)" % commit,
                   "left_out": unstable, "digests": digests}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("recorded %d cases from %s, left out %d: %s" % (len(digests), tree, len(unstable), unstable))


def _main(**kw):
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", required=True)
    ap.add_argument("--record", required=True)
    ap.add_argument("--commit", required=True, help="the parent commit that --tree is a checkout of")
    args = ap.parse_args()
    _record(args.tree, args.record, args.commit, **kw)


if __name__ == "__main__":
    _main()
