#!/usr/bin/env python3
"""Development aid: sha256 of the weights and the RMSProp slots after a few production train steps at the given row counts,
uint8 and f32 states.  Compare two builds or two settings (section 8b of DESIGN.md) by their lines: a change that only
moves work must print the same digests.
--net mlp | dmlp | ddpg: the vector-state networks instead: every arena and a prediction after three train steps at each
row count, on handles of (S, A) = (1, 1) and (64, 32) under every switch that picks other kernels, with the last step's
losses (ddpg: Q_max, and the slots of one prioritised step drawn from a ring of 1,025 rows).  --tree DIR: the package of
another built checkout.
usage: python tools/ab_bits.py [--net mlp|dmlp|ddpg] [--tree DIR] [rows ...]      (default 129 132 133; with --net 1 15 16 17 33)"""
import argparse
import hashlib
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def digest(arrays):
    h = hashlib.sha256()
    for t in arrays:
        h.update(np.ascontiguousarray(t).tobytes())
    return h.hexdigest()[:32]


def vector_net(net_kind, rows):
    from Config import Config
    dims = ((1, 1), (64, 32))
    if net_kind == "mlp":
        from NetworkVP_vector import Network
        cases = [((S, A), {"USE_GRAD_CLIP": clip, "DUAL_RMSPROP": dual})
                 for (S, A), dual, clip in itertools.product(dims, (False, True), (False, True))]
    else:       # chained widths 256, 129, 128, 3, 1: the shared backward splits a row over 1, 1, 2, 64 and 256 threads
        from NetworkVP_discrate import Network
        cases = [(d, {"DENSE_LAYERS": layers, "DENSE_STACK": stack, "USE_LOG_SOFTMAX": ls, "USE_GRAD_CLIP": clip})
                 for (d, layers, stack), ls, clip in itertools.product((((64, 32), (256, 129, 128, 3, 1), "chained"),
                                                                        ((1, 1), (10,), "fork")), (False, True), (False, True))]
    for (S, A), switches in cases:
        for k, v in switches.items():
            setattr(Config, k, v)
        net = Network("gpu:0", "ab_bits", A, (S,), max_batch=max(rows), predict_lanes=1)
        net.learning_rate, net.beta = 3e-4, 0.01
        for B in rows:
            rng = np.random.Generator(np.random.PCG64(B))
            x = rng.uniform(-1, 1, (B, S)).astype(np.float32)
            y = rng.uniform(-1, 1, B).astype(np.float32)
            a = (rng.uniform(-1, 1, (B, A)) if net_kind == "mlp" else np.eye(A)[rng.integers(0, A, B)]).astype(np.float32)
            for _ in range(3):
                net.train(x, y, a)
            arenas = [net.get_arena(i) for i in range(7 if switches.get("DUAL_RMSPROP") else 4)] + list(net.predict_p_and_v(x))
            print("%s S %d A %d %s rows %d %s losses %s" % (net_kind, S, A, " ".join("%s=%s" % kv for kv in switches.items()), B,
                                                          digest(arenas), net.last_losses.tobytes().hex()), flush=True)
        net.close()


def ddpg(rows):
    from Config import Config
    from NetworkDDPG import Network
    Config.add_OUnoise = False
    for (S, A), loss, clip, rms in itertools.product(((1, 1), (64, 32)), ("fork", "paired"), (False, True), (True, False)):
        Config.DDPG_CRITIC_LOSS, Config.USE_GRAD_CLIP, Config.RMSPROP = loss, clip, rms
        Config.PRIORITIZED_REPLAY = loss == "paired"
        net = Network("gpu:0", "ab_bits", A, (S,), max_batch=max(rows + [33]), predict_lanes=1, replay_capacity=2048)
        net.learning_rate = 1.0
        names = list(net.get_variables_names())
        tag = "ddpg S %d A %d loss=%s clip=%s critic=%s" % (S, A, loss, clip, "rmsprop" if rms else "adam")

        def draw(rng, B):
            return (rng.uniform(-1, 1, (B, S)), rng.uniform(-1, 1, (B, A)), rng.uniform(-1, 0, B), rng.uniform(size=B) < 0.1,
                    rng.uniform(-1, 1, (B, S)))

        def state():
            return digest(net.get_variable_value(k, which) for which in range(5) for k in names)

        for B in rows:
            s, a, r, done, s2 = draw(np.random.Generator(np.random.PCG64(B)), B)
            for _ in range(3):
                q = net.train(s, r, a, s2, done, noise=np.full(A, 0.25, np.float32))
            print("%s rows %d %s predict %s q_max %s" % (tag, B, state(), digest([net.predict(s, noise=False)]),
                                                         np.float32(q[0]).tobytes().hex()), flush=True)
        if net.prioritized:      # 1,025 rows: two chunks of priorities, the second holding one row
            rng = np.random.Generator(np.random.PCG64(1025))
            for n in [32] * 32 + [1]:
                net.replay_add(*draw(rng, n))
            net.train_prioritized(33, noise=np.full(A, 0.25, np.float32))
            print("%s prioritised rows 33 of 1025 %s slots %s" % (tag, state(), " ".join(str(t) for t in net.last_slots)), flush=True)
        net.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--net", choices=("image", "mlp", "dmlp", "ddpg"), default="image")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("rows", type=int, nargs="*")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import ga3c_amd  # noqa: F401
    if args.net != "image":
        rows = args.rows or [1, 15, 16, 17, 33]
        return ddpg(rows) if args.net == "ddpg" else vector_net(args.net, rows)
    from NetworkVP import Network
    rows = args.rows or [129, 132, 133]
    for B in rows:
        for u8 in (False, True):
            net = Network("gpu:0", "ab_bits", 6, (84, 84, 4), max_batch=B, predict_lanes=1)
            rng = np.random.Generator(np.random.PCG64(B))
            xk = rng.integers(0, 256, size=(B, 84, 84, 4), dtype=np.uint8)
            x = xk if u8 else xk.astype(np.float32) / np.float32(128) - np.float32(1)
            a = np.eye(6, dtype=np.float32)[rng.integers(0, 6, B)]
            y = rng.uniform(-1, 1, B).astype(np.float32)
            net.learning_rate, net.beta = 3e-4, 0.01
            for _ in range(3):
                net.train(x, y, a)
            print("rows %d %s %s" % (B, "u8 " if u8 else "f32", digest([net.get_arena(0), net.get_arena(1)])), flush=True)
            net.close()


if __name__ == "__main__":
    main()
