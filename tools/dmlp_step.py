#!/usr/bin/env python3
"""Development aid: step times of the discrete-action vector-state network (GAME = 'CartPole-v0', ga3c_dmlp_*), inputs
resident on the device, device-synchronised timing (ga3c_dmlp_time_resident: HIP events around `iters` back-to-back steps;
mode 0 = predict, 1 = train).  Median and min over rounds, one JSON line per configuration.  Launches per step: predict 1,
train 2 (3 with USE_GRAD_CLIP).  tools/mlp_step.py is the same measurement of the continuous vector-state network.
usage: python tools/dmlp_step.py [--predict 1 128] [--train 128 132 201] [--layers 10 10 10 10] [--chained] [--clip]
                                 [--rounds 5] [--iters 200]"""
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
    ap.add_argument("--state-dim", type=int, default=4)
    ap.add_argument("--actions", type=int, default=2)
    ap.add_argument("--layers", type=int, nargs="+", default=[10, 10, 10, 10])
    ap.add_argument("--chained", action="store_true")
    ap.add_argument("--clip", action="store_true")
    args = ap.parse_args()
    import ga3c_amd  # noqa: F401
    from Config import Config
    from NetworkVP_discrate import Network
    Config.USE_GRAD_CLIP = args.clip
    Config.DENSE_LAYERS = tuple(args.layers)
    Config.DENSE_STACK = 'chained' if args.chained else 'fork'
    S, A = args.state_dim, args.actions
    maxB = max(args.predict + args.train)
    net = Network("gpu:0", "dmlp_step", A, (S,), max_batch=maxB)
    rng = np.random.Generator(np.random.PCG64(1))
    x = rng.uniform(-1, 1, (maxB, S)).astype(np.float32)
    y = rng.uniform(-1, 1, maxB).astype(np.float32)
    a = np.eye(A, dtype=np.float32)[rng.integers(0, A, maxB)]
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
                          "layers": list(args.layers), "stack": Config.DENSE_STACK, "params": net.param_count,
                          "grad_clip": bool(args.clip), "launches": (3 if args.clip else 2) if mode else 1,
                          "median_us": round(v[len(v) // 2], 2), "min_us": round(v[0], 2), "max_us": round(v[-1], 2),
                          "rounds": args.rounds, "iters": args.iters}), flush=True)
    net.close()


if __name__ == "__main__":
    main()
