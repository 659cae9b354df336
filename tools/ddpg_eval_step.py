#!/usr/bin/env python3
"""Development aid: what one evaluation of the DDPG handle costs (ga3c_ddpg_eval_run; profiles/ddpg_eval.txt).
eval: eval_run(200) at each --envs, the kernel between two HIP events on the handle's stream ("elapsed_ms") and the wall clock
around the call, median / min / max of --rounds after one warm-up.
bar: the stepwise path it stands in for, 200 actor steps of the device actors without training and without noise
(actors_run(50, train=False) four times; a call takes at most 64 steps), wall clock around the four calls.  It needs nothing of
the evaluation entries, so it runs on a build without them too.
One JSON line per N.
usage: python tools/ddpg_eval_step.py eval|bar [--envs 16 64 256 4096] [--rounds 5]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = 200


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("eval", "bar"))
    ap.add_argument("--envs", type=int, nargs="+", default=[16, 64, 256, 4096])
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import ga3c_amd  # noqa: F401
    from NetworkDDPG import Network
    for n in args.envs:
        net = Network("gpu:0", "ddpg_eval_step", 1, (3,), max_batch=max(n, 64), predict_lanes=1, replay_capacity=max(n, 1024))
        if args.mode == "eval":
            net.eval_create(n, seed=1)
        else:
            net.actors_create(n, seed=1, batch=64)
            net.actors_run(1, train=False, noise=False)     # step(None)
        kernel, wall = [], []
        for r in range(args.rounds + 1):
            t0 = time.perf_counter()
            if args.mode == "eval":
                net.eval_run(STEPS)
            else:
                for _ in range(4):
                    net.actors_run(STEPS // 4, train=False, noise=False)
            if r:                                           # the first round warms up
                wall.append(1e3 * (time.perf_counter() - t0))
                if args.mode == "eval":
                    kernel.append(net.eval_get("elapsed_ms"))
            if args.mode == "bar":
                net.actors_episodes()
        wall.sort()
        kernel.sort()
        out = {"mode": args.mode, "n": n, "steps": STEPS, "rounds": args.rounds, "wall_ms_median": round(wall[len(wall) // 2], 3),
               "wall_ms_min": round(wall[0], 3), "wall_ms_max": round(wall[-1], 3)}
        if kernel:
            out.update(kernel_ms_median=round(kernel[len(kernel) // 2], 3), kernel_ms_min=round(kernel[0], 3),
                       kernel_ms_max=round(kernel[-1], 3))
        print(json.dumps(out), flush=True)
        net.close()


if __name__ == "__main__":
    main()
