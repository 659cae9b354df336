#!/usr/bin/env python3
"""Development aid: agent steps per second of the device actors (Config.DEVICE_AGENTS; ga3c_dmlp_actors_run for --game
CartPole-v0; ga3c_mlp_actors_run for --game Pendulum-v0) with training on -- every step a prediction for N environments, the actor step, the compaction and, when the step cut a
rollout, a train step on the cut rows.  Wall-clock around <prefix>_actors_run (the call returns when its steps are done:
the host reads a row count per step), median and min over rounds, one JSON line per N.  The figure to set it against is the
PPS of the status line of `_train.sh GAME=<game> AGENTS=16` (profiles/device_agents_step.txt, device_agents_pendulum.txt).
Pendulum's environments run in lockstep: one train step of N (TIME_MAX + 1) rows every TIME_MAX actor steps.
--ddpg (with --game Pendulum-v0; Config.DEVICE_DDPG, ga3c_ddpg_actors_run): the DDPG handle's actors, --updates
train steps of --batch ring rows after every actor step, --prioritized for the draw by priority, --nstep N for n-step returns
(Config.DDPG_NSTEP; profiles/nstep_step.txt); the call waits once, at its end (profiles/device_agents_ddpg.txt);
--eval-envs E --eval-every K for an evaluation of E noise-free episodes whenever the train steps pass a multiple of K, as
ThreadDeviceAgents runs them under DEVICE_DDPG_EVAL_ENVS (profiles/ddpg_eval.txt), inside the timed rounds;
--noise per_env for every environment's own noise process (Config.DEVICE_DDPG_NOISE; profiles/envnoise_step.txt);
--action-bound, --time-limit, --reset-observation, --reward-scale, --reward-offset for the actors' task (Config.DEVICE_DDPG_ACTION_BOUND
and its neighbours; profiles/ddpg_task_step.txt): any non-default one attaches a task (without one the handle steps under the fork's values).
usage: python tools/device_agents_step.py [--game CartPole-v0|Pendulum-v0] [--agents 256 4096] [--time-max 5] [--steps 64] [--calls 8] [--rounds 5] [--no-train]
       [--ddpg [--batch 64] [--updates 1] [--prioritized] [--capacity 1000000] [--nstep 1] [--eval-envs 0] [--eval-every 1000] [--noise shared|per_env]
        [--action-bound wrap|clip] [--time-limit terminal|truncate] [--reset-observation] [--reward-scale 0.005] [--reward-offset -1]]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--game", choices=("CartPole-v0", "Pendulum-v0"), default="CartPole-v0")
    ap.add_argument("--agents", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--time-max", type=int, default=5)
    ap.add_argument("--steps", type=int, default=64, help="actor steps per native call (1..64)")
    ap.add_argument("--calls", type=int, default=8, help="native calls per round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-train", action="store_true")
    ap.add_argument("--ddpg", action="store_true", help="the DDPG handle's actors (Pendulum-v0)")
    ap.add_argument("--batch", type=int, default=64, help="--ddpg: rows of a train step")
    ap.add_argument("--updates", type=int, default=1, help="--ddpg: train steps per actor step")
    ap.add_argument("--prioritized", action="store_true", help="--ddpg: draw by priority (paired critic loss)")
    ap.add_argument("--capacity", type=int, default=1000000, help="--ddpg: ring slots")
    ap.add_argument("--nstep", type=int, default=1, help="--ddpg: steps of the returns the actors write (1..16)")
    ap.add_argument("--eval-envs", type=int, default=0, help="--ddpg: evaluation environments (0: none)")
    ap.add_argument("--eval-every", type=int, default=1000, help="--ddpg: train steps between two evaluations")
    ap.add_argument("--noise", choices=("shared", "per_env"), default="shared", help="--ddpg: the actors' exploration noise")
    ap.add_argument("--action-bound", choices=("wrap", "clip"), default="wrap", help="--ddpg: DEVICE_DDPG_ACTION_BOUND")
    ap.add_argument("--time-limit", choices=("terminal", "truncate"), default="terminal", help="--ddpg: DEVICE_DDPG_TIME_LIMIT")
    ap.add_argument("--reset-observation", action="store_true", help="--ddpg: DEVICE_DDPG_RESET_OBSERVATION")
    ap.add_argument("--reward-scale", type=float, default=0.005, help="--ddpg: DEVICE_DDPG_REWARD_SCALE")
    ap.add_argument("--reward-offset", type=float, default=-1.0, help="--ddpg: DEVICE_DDPG_REWARD_OFFSET")
    args = ap.parse_args()
    import ga3c_amd  # noqa: F401
    from Config import Config
    if args.ddpg:
        if args.game != "Pendulum-v0":
            ap.error("--ddpg steps Pendulum-v0")
        from NetworkDDPG import Network
        num_actions, state_dim = 1, (3,)
        Config.PRIORITIZED_REPLAY = args.prioritized
        Config.DDPG_NSTEP = args.nstep
        Config.DEVICE_DDPG_NOISE = args.noise
        Config.DEVICE_DDPG_ACTION_BOUND, Config.DEVICE_DDPG_TIME_LIMIT = args.action_bound, args.time_limit
        Config.DEVICE_DDPG_RESET_OBSERVATION = args.reset_observation
        Config.DEVICE_DDPG_REWARD_SCALE, Config.DEVICE_DDPG_REWARD_OFFSET = args.reward_scale, args.reward_offset
        if args.prioritized:
            Config.DDPG_CRITIC_LOSS = 'paired'
    elif args.game == "Pendulum-v0":
        from NetworkVP_vector import Network
        num_actions, state_dim = 1, (3,)
    else:
        from NetworkVP_discrate import Network
        num_actions, state_dim = 2, (4,)
    for n in args.agents:
        if args.ddpg:
            net = Network("gpu:0", "device_agents_step", num_actions, state_dim, max_batch=max(n, args.batch), predict_lanes=1,
                          replay_capacity=args.capacity)
            net.learning_rate = Config.LEARNING_RATE_START
            net_task = list(net.task) if net.task else None
            net.actors_create(n, seed=Config.RANDOM_SEED, updates=args.updates, batch=args.batch)
            if args.eval_envs:
                net.eval_create(args.eval_envs)
        else:
            net = Network("gpu:0", "device_agents_step", num_actions, state_dim, max_batch=max(16, n * (args.time_max + 1)), predict_lanes=1)
            net.learning_rate, net.beta = Config.LEARNING_RATE_START, Config.BETA_START
            net.actors_create(n, args.time_max, Config.DISCOUNT, Config.RANDOM_SEED)
        net.actors_run(args.steps, train=not args.no_train)               # warm-up; the rollouts are in step from here on
        rates, train_rates, train_calls, rows, episodes, evaluations = [], [], 0, 0, 0, 0
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            steps, calls0 = 0, train_calls
            for _ in range(args.calls):
                s, c, r, e = net.actors_run(args.steps, train=not args.no_train)
                if args.ddpg and args.eval_envs and (train_calls + c) // args.eval_every > train_calls // args.eval_every:
                    net.eval_run(200)
                    evaluations += 1
                steps, train_calls, rows, episodes = steps + s, train_calls + c, rows + r, episodes + e
            rates.append(steps / (time.perf_counter() - t0))
            train_rates.append((train_calls - calls0) / (time.perf_counter() - t0))
            net.actors_episodes()
        rates.sort()
        per_step_us = 1e6 * n / rates[len(rates) // 2]
        extra = ({"ddpg": True, "batch": args.batch, "updates": args.updates, "prioritized": args.prioritized, "nstep": args.nstep,
                  "noise": args.noise, "task": net_task,
                  "eval_envs": args.eval_envs, "eval_every": args.eval_every, "evaluations": evaluations,
                  "train_steps_per_s_median": round(sorted(train_rates)[len(train_rates) // 2])} if args.ddpg else {})
        print(json.dumps({**extra, "game": args.game, "agents": n, "time_max": args.time_max, "train": not args.no_train, "steps_per_call": args.steps,
                          "agent_steps_per_s_median": round(rates[len(rates) // 2]), "agent_steps_per_s_min": round(rates[0]),
                          "agent_steps_per_s_max": round(rates[-1]), "actor_step_us_median": round(per_step_us, 1),
                          "train_calls": train_calls, "rows_trained": rows, "episodes": episodes, "rounds": args.rounds}),
              flush=True)
        net.close()


if __name__ == "__main__":
    main()
