#!/usr/bin/env python3
"""Development aid: what prioritised replay (Config.PRIORITIZED_REPLAY) adds to a DDPG train step.

  python tools/per_step.py [--batches 64 128 256] [--rings 65536 1048576] [--rounds 5] [--iters 200]
                           [--parent-tree DIR] [--record profiles/per_step.txt]
      Per ring (filled to its capacity, priorities U(0.01, 2)^0.6) and batch: ga3c_ddpg_time_prioritized (HIP events on the
      handle's stream around `iters` prioritised steps: draw, step, priority update, 8 launches) and, on the same handle,
      ga3c_ddpg_time_resident mode 1 (train_replay on slots 0 .. B-1, 5 launches), in alternating rounds; median / min of the
      rounds in us per step, one JSON line each.  --parent-tree: a built checkout of the commit before prioritised replay;
      its tools/ddpg_step.py is run beside, in the same visit, for the step this change must not have slowed.
  python tools/per_step.py --steps-only [--rings 1048576] [--batches 64] [--iters 200]
      Prioritised steps and nothing else, for `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python ...`.
  python tools/per_step.py --digest DIR [--record ...]
      The per-kernel lines of that run's kernel_stats.csv (calls, average / min / max time).
Every command and every line printed is appended to --record."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Record:
    def __init__(self, path):
        self.f = open(path, "a") if path else None

    def __call__(self, line):
        print(line, flush=True)
        if self.f:
            self.f.write(line + "\n")
            self.f.flush()


def filled(ring, max_batch=4096):
    """-> a DDPG handle with priorities whose ring of `ring` slots is full."""
    import ga3c_amd  # noqa: F401
    from Config import Config
    from NetworkDDPG import Network
    Config.PRIORITIZED_REPLAY, Config.DDPG_CRITIC_LOSS = True, 'paired'
    S, A = 3, 1
    net = Network("gpu:0", "per_step", A, (S,), max_batch=max_batch, replay_capacity=ring)
    rng = np.random.Generator(np.random.PCG64(1))
    for lo in range(0, ring, max_batch):
        n = min(max_batch, ring - lo)
        net.replay_add(rng.uniform(-1, 1, (n, S)), rng.uniform(-1, 1, (n, A)), rng.uniform(-1, 0, n),
                       rng.uniform(size=n) < 0.1, rng.uniform(-1, 1, (n, S)))
    net.set_priorities(rng.uniform(0.01, 2, ring).astype(np.float32) ** np.float32(0.6), 2.0)
    net.learning_rate = 1e-6
    net.replay_beta = 0.4
    return net


def measure(args, rec):
    for ring in args.rings:
        net = filled(ring)
        jobs = [(kind, b) for b in args.batches for kind in ("train_prioritized", "train_replay")]
        res = {j: [] for j in jobs}

        def run(kind, b, iters):
            return net.time_prioritized(b, iters) if kind == "train_prioritized" else net.time_resident(1, b, iters)
        for kind, b in jobs:
            run(kind, b, 20)                              # warm-up
        for _ in range(args.rounds):
            for kind, b in jobs:
                res[(kind, b)].append(run(kind, b, args.iters) / args.iters * 1e3)
        for (kind, b), v in res.items():
            v = sorted(v)
            rec(json.dumps({"step": kind, "ring": ring, "rows": b, "launches": 8 if kind == "train_prioritized" else 5,
                            "median_us": round(v[len(v) // 2], 2), "min_us": round(v[0], 2), "rounds": args.rounds,
                            "iters": args.iters}))
        for b in args.batches:
            extra = sorted(res[("train_prioritized", b)])[args.rounds // 2] - sorted(res[("train_replay", b)])[args.rounds // 2]
            rec("# ring %d rows %d: the prioritised step costs %.2f us more than train_replay on this build" % (ring, b, extra))
        net.close()
    if args.parent_tree:
        cmd = [sys.executable, os.path.join(args.parent_tree, "tools", "ddpg_step.py"), "--predict", "1", "--train"] + \
              [str(b) for b in args.batches] + ["--rounds", str(args.rounds), "--iters", str(args.iters)]
        rec("# the parent commit, built beside: " + " ".join(["python", "<parent>/tools/ddpg_step.py"] + cmd[2:]))
        out = subprocess.run(cmd, cwd=args.parent_tree, stdout=subprocess.PIPE, check=True).stdout.decode()
        for line in out.splitlines():
            if '"train_replay"' in line:
                rec(line)


def steps_only(args):
    for ring in args.rings:
        net = filled(ring)
        for b in args.batches:
            net.time_prioritized(b, args.iters)
        net.close()


def digest(args, rec):
    found = sorted(glob.glob(os.path.join(args.digest, "**", "*kernel_stats.csv"), recursive=True))
    if not found:
        raise SystemExit("no kernel_stats.csv under " + args.digest)
    for r in csv.DictReader(open(found[0])):
        name = r["Name"].split("(")[0].replace("ga3c_dd::", "").replace("void ", "")
        if name.startswith(("per_", "ddpg_")):
            rec("%-28s calls %5d  avg %8.1f us  min %8.1f us  max %8.1f us" % (
                name, int(r["Calls"]), float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--rings", type=int, nargs="+", default=[65536, 1048576])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--parent-tree")
    ap.add_argument("--record")
    ap.add_argument("--steps-only", action="store_true")
    ap.add_argument("--digest")
    args = ap.parse_args()
    rec = Record(args.record)
    if args.steps_only:
        return steps_only(args)
    rec("# python tools/per_step.py " + " ".join(a if not os.path.isabs(a) else "<dir>" for a in sys.argv[1:]))
    if args.digest:
        return digest(args, rec)
    measure(args, rec)


if __name__ == "__main__":
    main()
