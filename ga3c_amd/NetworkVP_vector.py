"""Network for vector-state games (Config.GAME = 'Pendulum-v0') -- the network the reference fork itself trains
(/root/reference/ga3c/NetworkVP.py:67-105,164-210), backed by the ga3c_mlp handle of libga3c_hip.so.

    x[B,S] -> dense11_p (4) -> dense12_p (256) -> dense13_p (256) -> dense14_p (100, sigmoid) -> dense1 (64, sigmoid)
           -> logits_v (1) and the angle-output head logits_p/out_x, out_y (A each, sigmoid): p = atan2(Y, X) / pi

The interface is NetworkVP_vecnet.VectorNetwork's; this module states the layer table, the initial weights and what
ga3c_mlp_create and ga3c_mlp_evaluate take.
"""
import numpy as np

from Config import Config
from NetworkVP_vecnet import DeviceActors, VectorNetwork
import _native as nat

TRUNK = (("dense11_p", 4), ("dense12_p", 256), ("dense13_p", 256), ("dense14_p", 100), ("dense1", 64))
HEADS = ("logits_v", "logits_p/out_x", "logits_p/out_y")
INIT = 0.3                  # dense_layer's U(-0.3, 0.3), weights and biases alike (NetworkVP.py:194-204)
# what ga3c_mlp_actors_get names, per environment: dtype and elements ("batch_*": rows of the last step's batch instead).
# "phys" is (th, thdot); "action" is the action vector, the prediction row the step took; "u" stays -1: no draw for an action
ACTOR_FIELDS = {"phys": (np.float64, 2), "elapsed": (np.int32, 1), "time_count": (np.int32, 1), "started": (np.int32, 1),
                "draws": (np.uint64, 1), "obs": (np.float32, "S"), "p": (np.float32, "A"), "v": (np.float32, 1),
                "u": (np.float64, 1), "action": (np.float32, "A"), "reward": (np.float64, 1), "done": (np.int32, 1),
                "cut": (np.int32, 1), "rollout_len": (np.int32, 1),
                "batch_x": (np.float32, "S"), "batch_y_r": (np.float32, 1), "batch_a": (np.float32, "A")}


def param_order():
    return tuple("%s/%s" % (layer, wb) for layer in [t[0] for t in TRUNK] + list(HEADS) for wb in ("w", "b"))


def param_shapes(state_dim, num_actions):
    shapes, fan_in = {}, int(state_dim)
    for name, width in TRUNK:
        shapes[name + "/w"], shapes[name + "/b"] = (fan_in, width), (width,)
        fan_in = width
    for name, width in zip(HEADS, (1, num_actions, num_actions)):
        shapes[name + "/w"], shapes[name + "/b"] = (fan_in, width), (width,)
    return shapes


def initial_arena(state_dim, num_actions, seed):
    """U(-0.3, 0.3) for every variable, drawn from one PCG64(seed) stream in variable order."""
    rng = np.random.Generator(np.random.PCG64(seed))
    shapes = param_shapes(state_dim, num_actions)
    return np.concatenate([rng.uniform(-INIT, INIT, size=shapes[k]).astype(np.float32).ravel() for k in param_order()])


class Network(DeviceActors, VectorNetwork):
    PREFIX = "ga3c_mlp"
    LOGITS_PER_ACTION = 2         # z = [hx | hy]
    ACTIVATION_WIDTHS = (4, 256, 64)                                              # pd1, pd2, d1
    ACTIVATION_TAGS = ("activation_pd1", "activation_pd2", "activation_d2")      # NetworkVP.py:150-170
    DUAL_RMSPROP_REFUSAL = None   # Config.DUAL_RMSPROP: one optimizer per cost, arenas 4 / 5 / 6
    ACTOR_FIELDS = ACTOR_FIELDS   # device actors (Config.DEVICE_PENDULUM): ga3c_mlp_actors_*, Pendulum-v0
    ACTOR_SCALARS = {"batch_rows": np.int32}
    ACTOR_ROWS = dict.fromkeys(("batch_x", "batch_y_r", "batch_a"), "batch_rows")

    def _config(self):
        cfg = nat.MlpConfig()
        cfg.flags = nat.FLAG_CONTINUOUS | (nat.FLAG_GRAD_CLIP if Config.USE_GRAD_CLIP else 0) | \
            (nat.FLAG_DUAL_RMSPROP if Config.DUAL_RMSPROP else 0)
        return cfg

    def _variables(self):
        return (param_order(), param_shapes(self.S, self.num_actions),
                initial_arena(self.S, self.num_actions, Config.RANDOM_SEED))
