#!/usr/bin/env python3
"""Development aid: the learning curve of one DDPG variant on Pendulum-v0.  Drives NetworkDDPG.Network directly,
with no Server: --actors device actors (Config.DEVICE_DDPG's loop, actors_run(32) at a time, one train step of --batch rows per
actor step once the ring holds more than a batch), and every --every train steps a noise-free evaluation of --eval-envs episodes
of 200 steps from fixed start states (eval_run; one more before the first train step).  The variant is given as the product's
own KEY=VALUE settings and checked by the product's resolvers; --noise per_env is DEVICE_DDPG_NOISE=per_env.  Writes <out-dir>/<name>.csv,
    training_step, n, steps, mean, min, max, mean_gym_return, wall_s
(mean_gym_return = (mean - steps * offset) / scale undoes the reward's DEVICE_DDPG_REWARD_SCALE and _OFFSET, the wrapper's
r * 0.005 - 1 at the defaults: gym's number for Pendulum-v0, 0 at best and about -1200 to -1500 for a policy that
does nothing), and prints one JSON line: the first evaluation, the best, the mean of the last
five, the wall time.  profiles/learning_curves.md is the record of the variants that exist.
usage: python tools/learning_curve.py --name paired [--train-steps 60000] [--every 1000] [--actors 256] [--batch 64]
       [--eval-envs 64] [--noise shared|per_env] [--out-dir profiles/learning_curves] DDPG_CRITIC_LOSS=paired ..."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
EVAL_STEPS = 200
CHUNK = 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--name", required=True)
    ap.add_argument("--train-steps", type=int, default=60000)
    ap.add_argument("--every", type=int, default=1000)
    ap.add_argument("--actors", type=int, default=256)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--eval-envs", type=int, default=64)
    ap.add_argument("--noise", choices=("shared", "per_env"), default=None, help="DEVICE_DDPG_NOISE, unless the settings give it")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "learning_curves"))
    ap.add_argument("settings", nargs="*", help="KEY=VALUE, as GA3C.py takes them")
    args = ap.parse_args()
    import ga3c_amd  # noqa: F401
    from Config import Config, resolve_device_agents
    import GA3C
    Config.GAME, Config.USE_DDPG, Config.DEVICE_DDPG = 'Pendulum-v0', True, True
    Config.DEVICE_AGENTS, Config.TRAINING_MIN_BATCH_SIZE = args.actors, args.batch
    Config.DEVICE_DDPG_EVAL_ENVS, Config.DEVICE_DDPG_EVAL_EVERY = args.eval_envs, args.every
    if args.noise is not None:
        Config.DEVICE_DDPG_NOISE = args.noise
    GA3C.apply_argv(args.settings)              # the variant, coerced and resolved as the product does
    resolve_device_agents()
    from NetworkDDPG import FORK_TASK, Network
    net = Network("gpu:0", "learning_curve_" + args.name, 1, (3,), max_batch=max(args.actors, args.batch), predict_lanes=1)
    net.learning_rate = Config.LEARNING_RATE_START
    net.actors_create(args.actors)
    net.eval_create(args.eval_envs)
    os.makedirs(args.out_dir, exist_ok=True)
    path = os.path.join(args.out_dir, args.name + ".csv")
    rows, trained, t0 = [], 0, time.perf_counter()

    def evaluate(out):
        totals = net.eval_run(EVAL_STEPS, bool(Config.DEVICE_DDPG_EVAL_TARGET))
        mean = float(totals.mean())
        scale, offset = (net.task or FORK_TASK)[3:]       # what the handle holds, as log_eval reads it
        rows.append((mean - EVAL_STEPS * offset) / scale)
        out.write("%d,%d,%d,%.17g,%.17g,%.17g,%.17g,%.3f\n" % (trained, totals.size, EVAL_STEPS, mean, float(totals.min()),
                                                              float(totals.max()), rows[-1], time.perf_counter() - t0))
        out.flush()

    with open(path, "w") as out:
        evaluate(out)
        done = 0
        while trained < args.train_steps:
            trained += net.actors_run(CHUNK)[1]
            net.actors_episodes()               # the exploring policy's records: not this tool's subject
            if trained // args.every > done:
                done = trained // args.every
                evaluate(out)
    wall = time.perf_counter() - t0
    net.eval_destroy()
    net.actors_destroy()
    net.close()
    last = rows[-5:]
    print(json.dumps({"name": args.name, "settings": args.settings, "train_steps": trained, "evaluations": len(rows),
                      "first_gym_return": round(rows[0], 1), "best_gym_return": round(max(rows), 1),
                      "best_at_evaluation": rows.index(max(rows)), "last5_mean_gym_return": round(sum(last) / len(last), 1),
                      "wall_s": round(wall, 1), "csv": os.path.relpath(path, ROOT)}), flush=True)


if __name__ == "__main__":
    main()
