#!/usr/bin/env python3
"""Development aid: step times of the DDPG handle (USE_DDPG, ga3c_ddpg_*), rows resident in the replay ring, device-
synchronised timing (ga3c_ddpg_time_resident: HIP events around `iters` back-to-back calls on ring slots 0 .. rows-1;
mode 0 = predict, 1 = train_replay).  Median and min over rounds, one JSON line per configuration.  Launches per call:
predict 1, train_replay 5 (6 with USE_GRAD_CLIP).  --twin: the handle has twin critics (DDPG_TWIN) and a step that
is not a policy step is 3 launches (4), so the time is the mean over --delay steps; --delay 1 times the policy step.
--nstep N > 1: the handle has n-step state (DDPG_NSTEP) and the target kernel reads a discount per ring slot.
--dist: the handle has a distributional critic (DDPG_DISTRIBUTIONAL) of --atoms atoms; the launches are the same.
--soft: the twin handle has the soft actor-critic (DDPG_SOFT; implies --twin); the launches are the twin's.
KEY=VALUE: the product's own settings, applied after the flags and checked by the product's resolvers, e.g. DDPG_CRITIC_LOSS=paired
or DDPG_CRITIC_LOSS=paired DDPG_POPART=True (one more launch, a single workgroup).
usage: python tools/ddpg_step.py [--predict 1 128] [--train 64 128 256] [--rounds 5] [--iters 200] [--clip] [--twin [--delay N]]
       [--soft] [--nstep N] [--dist [--atoms N]] [KEY=VALUE ...]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--predict", type=int, nargs="+", default=[1, 128])
    ap.add_argument("--train", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--state-dim", type=int, default=3)
    ap.add_argument("--actions", type=int, default=1)
    ap.add_argument("--clip", action="store_true")
    ap.add_argument("--twin", action="store_true")
    ap.add_argument("--delay", type=int, default=2)
    ap.add_argument("--soft", action="store_true")
    ap.add_argument("--nstep", type=int, default=1)
    ap.add_argument("--dist", action="store_true")
    ap.add_argument("--atoms", type=int, default=51)
    ap.add_argument("settings", nargs="*", help="KEY=VALUE, as GA3C.py takes them")
    args = ap.parse_args()
    import ga3c_amd  # noqa: F401
    from Config import Config
    from NetworkDDPG import Network
    Config.USE_GRAD_CLIP = args.clip
    if args.soft:
        args.twin, Config.DDPG_SOFT = True, True
    if args.twin:
        Config.DDPG_TWIN, Config.DDPG_CRITIC_LOSS, Config.DDPG_POLICY_DELAY = True, 'paired', args.delay
    Config.DDPG_NSTEP = args.nstep
    if args.dist:
        Config.DDPG_DISTRIBUTIONAL, Config.DDPG_CRITIC_LOSS, Config.DDPG_ATOMS = True, 'paired', args.atoms
    S, A = args.state_dim, args.actions
    maxB = max(args.predict + args.train)
    if args.settings:
        import GA3C
        Config.GAME, Config.USE_DDPG, Config.TRAINING_MIN_BATCH_SIZE = 'Pendulum-v0', True, maxB
        GA3C.apply_argv(args.settings)
    popart = bool(getattr(Config, "DDPG_POPART", False))
    net = Network("gpu:0", "ddpg_step", A, (S,), max_batch=maxB, replay_capacity=max(maxB, 1024))
    rng = np.random.Generator(np.random.PCG64(1))
    net.replay_add(rng.uniform(-1, 1, (maxB, S)), rng.uniform(-1, 1, (maxB, A)), rng.uniform(-1, 0, maxB),
                   rng.uniform(size=maxB) < 0.1, rng.uniform(-1, 1, (maxB, S)))
    net.learning_rate = 1e-6
    jobs = [(0, b) for b in args.predict] + [(1, b) for b in args.train]
    res = {j: [] for j in jobs}
    for mode, b in jobs:
        net.time_resident(mode, b, 20)                  # warm-up
    for _ in range(args.rounds):
        for mode, b in jobs:
            res[(mode, b)].append(net.time_resident(mode, b, args.iters) / args.iters * 1e3)
    for (mode, b), v in res.items():
        v = sorted(v)
        print(json.dumps({"step": "train_replay" if mode else "predict", "rows": b, "state_dim": S, "actions": A,
                          "grad_clip": bool(args.clip), "launches": (6 if args.clip else 5) + popart if mode else 1,
                          "critic_loss": Config.DDPG_CRITIC_LOSS, "popart": popart,
                          "nstep": args.nstep, "twin": bool(args.twin), "soft": bool(args.soft), "policy_delay": args.delay if args.twin else None,
                          "launches_off_policy_step": ((4 if args.clip else 3) if mode else 1) if args.twin else None,
                          "atoms": args.atoms if args.dist else None,
                          "median_us": round(v[len(v) // 2], 2), "min_us": round(v[0], 2), "max_us": round(v[-1], 2), "rounds": args.rounds,
                          "iters": args.iters}), flush=True)
    net.close()


if __name__ == "__main__":
    main()
