#!/usr/bin/env python3
"""Development aid: the DUAL_RMSPROP train step against the single-optimizer step at the same rows, inputs resident on the
device, device-synchronised timing (ga3c_net_time_resident: HIP events around `iters` back-to-back steps on the train
stream).  Interleaved rounds, median and min per configuration, one JSON line each.  Also prints the bytes the dual
update kernel (rmsprop_dual_kernel) must move per step, to turn its kernel time (rocprofv3 --kernel-trace --stats) into
a bandwidth.
usage: python tools/dual_step.py [--batch 128 132] [--rounds 7] [--iters 200] [--f32]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def update_bytes(num_actions, momentum):
    """Bytes rmsprop_dual_kernel reads and writes in one step: theta in / out, both gradients, each optimizer's ms (and
    mom) read and written where it has a slot, dense1/w's fragment-ordered copy and the packed conv filters."""
    n = 3872 * 256 + 256 + 8 * 8 * 4 * 16 + 16 + 4 * 4 * 16 * 32 + 32 + 257 + 257 * num_actions
    head_v, head_p = 257, 257 * num_actions
    slots_v, slots_p = n - head_p, n - head_v
    per_slot = 2 if momentum else 1
    floats = 2 * n + (slots_v + slots_p) + 2 * per_slot * (slots_v + slots_p)
    floats += 3872 * 256 + 8 * 8 * 4 * 16 + 4 * 4 * 16 * 32
    return 4 * floats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[128, 132])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--f32", action="store_true", help="f32-resident states (default: uint8, what the transport delivers)")
    ap.add_argument("--only-dual", action="store_true", help="no single-optimizer net (a profile of the dual step alone)")
    args = ap.parse_args()
    import ga3c_amd  # noqa: F401
    from Config import Config
    from NetworkVP import Network
    import _native as nat
    A = 6
    maxB = max(args.batch)
    nets = {}
    for dual in ((True,) if args.only_dual else (False, True)):
        Config.DUAL_RMSPROP = dual
        nets["dual" if dual else "single"] = Network("gpu:0", "dual_step", A, (84, 84, 4), max_batch=maxB, predict_lanes=1)
    Config.DUAL_RMSPROP = False
    rng = np.random.Generator(np.random.PCG64(1))
    res = {}
    ms = nat.C.c_float()
    for B in args.batch:
        xk = rng.integers(0, 256, size=(B, 84, 84, 4), dtype=np.uint8)
        x = xk.astype(np.float32) / np.float32(128) - np.float32(1)
        a = np.eye(A, dtype=np.float32)[rng.integers(0, A, B)]
        y = rng.uniform(-1, 1, B).astype(np.float32)
        for name, net in nets.items():
            net.learning_rate, net.beta = 3e-4, 0.01
            net.train(x, y, a)                   # every workspace buffer holds real data
            lib, h = net._lib, net._h
            if args.f32:
                nat.check(lib.ga3c_net_upload(h, nat.ptr(x), nat.ptr(y), nat.ptr(a), B))
            else:
                nat.check(lib.ga3c_net_upload_u8(h, nat.ptr(xk, nat.u8p), nat.ptr(y), nat.ptr(a), B))
            res[(name, B)] = []
        for _ in range(args.rounds):
            for name, net in nets.items():
                nat.check(net._lib.ga3c_net_time_resident(net._h, 1, B, args.iters, 3e-4, 0.01, nat.C.byref(ms)), name)
                res[(name, B)].append(ms.value / args.iters * 1e3)
    for (name, B), v in sorted(res.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        v = sorted(v)
        print(json.dumps({"step": name, "rows": B, "states": "f32" if args.f32 else "uint8", "median_us": round(v[len(v) // 2], 2),
                          "min_us": round(v[0], 2), "rounds": args.rounds, "iters": args.iters}))
    print(json.dumps({"dual_update_bytes": update_bytes(A, Config.RMSPROP_MOMENTUM != 0.0), "num_actions": A}))
    for net in nets.values():
        net.close()


if __name__ == "__main__":
    main()
