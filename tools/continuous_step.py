#!/usr/bin/env python3
"""Development aid: the CONTINUOUS_INPUT step times against the discrete step at the same rows and action counts, inputs
resident on the device, device-synchronised timing (ga3c_net_time_resident: HIP events around `iters` back-to-back steps;
mode 0 = predict, 1 = train).  Interleaved rounds, median and min per configuration, one JSON line each.
usage: python tools/continuous_step.py [--actions 1 3 6] [--batch 1 32 128 132] [--rounds 5] [--iters 200]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--actions", type=int, nargs="+", default=[1, 3, 6])
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 32, 128, 132])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    import ga3c_amd  # noqa: F401
    from Config import Config
    from NetworkVP import Network
    import _native as nat
    maxB = max(args.batch)
    rng = np.random.Generator(np.random.PCG64(1))
    ms = nat.C.c_float()
    for A in args.actions:
        nets = {}
        for cont in (False, True):
            Config.CONTINUOUS_INPUT = cont
            nets["continuous" if cont else "discrete"] = Network("gpu:0", "cont_step", A, (84, 84, 4), max_batch=maxB,
                                                                predict_lanes=1)
        Config.CONTINUOUS_INPUT = False
        for B in args.batch:
            xk = rng.integers(0, 256, size=(B, 84, 84, 4), dtype=np.uint8)
            y = rng.uniform(-1, 1, B).astype(np.float32)
            res = {}
            for name, net in nets.items():
                a = (rng.uniform(-1, 1, (B, A)).astype(np.float32) if name == "continuous"
                     else np.eye(A, dtype=np.float32)[rng.integers(0, A, B)])
                net.learning_rate, net.beta = 3e-4, 0.01
                net.train(xk, y, a)              # every workspace buffer holds real data
                nat.check(net._lib.ga3c_net_upload_u8(net._h, nat.ptr(xk, nat.u8p), nat.ptr(y), nat.ptr(a), B))
                for mode in (0, 1):
                    res[(name, mode)] = []
            for _ in range(args.rounds):
                for mode in (0, 1):
                    for name, net in nets.items():
                        nat.check(net._lib.ga3c_net_time_resident(net._h, mode, B, args.iters, 3e-4, 0.01, nat.C.byref(ms)),
                                  name)
                        res[(name, mode)].append(ms.value / args.iters * 1e3)
            for (name, mode), v in sorted(res.items(), key=lambda kv: (kv[0][1], kv[0][0])):
                v = sorted(v)
                print(json.dumps({"head": name, "step": "train" if mode else "predict", "actions": A, "rows": B,
                                  "states": "uint8", "median_us": round(v[len(v) // 2], 2), "min_us": round(v[0], 2),
                                  "rounds": args.rounds, "iters": args.iters}), flush=True)
        for net in nets.values():
            net.close()


if __name__ == "__main__":
    main()
