#!/usr/bin/env python3
"""Development aid: step times of the vector-state network (GAME = 'Pendulum-v0', ga3c_mlp_*), inputs resident on the
device, device-synchronised timing (ga3c_mlp_time_resident: HIP events around `iters` back-to-back steps; mode 0 =
predict, 1 = train).  Median and min over rounds, one JSON line per configuration.  Launches per step: predict 1, train 2
(3 with USE_GRAD_CLIP).
--dual: Config.DUAL_RMSPROP, one RMSProp optimizer per cost; the same launch counts.
usage: python tools/mlp_step.py [--predict 1 128] [--train 128 132 201] [--rounds 5] [--iters 200] [--clip] [--dual]"""
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
    ap.add_argument("--train", type=int, nargs="+", default=[128, 132, 201])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--state-dim", type=int, default=3)
    ap.add_argument("--actions", type=int, default=1)
    ap.add_argument("--clip", action="store_true")
    ap.add_argument("--dual", action="store_true")
    args = ap.parse_args()
    import ga3c_amd  # noqa: F401
    from Config import Config
    from NetworkVP_vector import Network
    Config.USE_GRAD_CLIP = args.clip
    Config.DUAL_RMSPROP = args.dual
    S, A = args.state_dim, args.actions
    maxB = max(args.predict + args.train)
    net = Network("gpu:0", "mlp_step", A, (S,), max_batch=maxB)
    rng = np.random.Generator(np.random.PCG64(1))
    x = rng.uniform(-1, 1, (maxB, S)).astype(np.float32)
    y = rng.uniform(-1, 1, maxB).astype(np.float32)
    a = rng.uniform(-1, 1, (maxB, A)).astype(np.float32)
    net.learning_rate, net.beta = 1e-6, 0.01
    net.upload(x, y, a)
    jobs = [(0, b) for b in args.predict] + [(1, b) for b in args.train]
    res = {j: [] for j in jobs}
    for mode, b in jobs:
        net.time_resident(mode, b, 20)                  # warm-up
    for _ in range(args.rounds):
        for mode, b in jobs:
            res[(mode, b)].append(net.time_resident(mode, b, args.iters) / args.iters * 1e3)
    for (mode, b), v in res.items():
        v = sorted(v)
        print(json.dumps({"step": "train" if mode else "predict", "rows": b, "state_dim": S, "actions": A,
                          "grad_clip": bool(args.clip), "dual_rmsprop": bool(args.dual), "launches": (3 if args.clip else 2) if mode else 1,
                          "median_us": round(v[len(v) // 2], 2), "min_us": round(v[0], 2), "rounds": args.rounds,
                          "iters": args.iters}), flush=True)
    net.close()


if __name__ == "__main__":
    main()
