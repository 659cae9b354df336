"""Network for vector-state games with a discrete action space (Config.GAME = 'CartPole-v0') -- the reference's third
network class (ga3c/NetworkVP_discrate.py:39-146; the module name is the reference's, sic), backed by the ga3c_dmlp handle
of libga3c_hip.so.

    x[B,S] -> dense1_<i>_p (Config.DENSE_LAYERS[i - 1] units, sigmoid), i = 1..L -> logits_v (1) and logits_p (A) -> softmax

Config.DENSE_STACK = 'fork' builds the layers as the reference does (:52-56): every one of them reads x and only the last
reaches the heads, so dense1_1_p .. dense1_<L-1>_p are variables that nothing reads -- created, initialised, saved and
histogrammed, never trained.  'chained' feeds layer i - 1 into layer i.

The interface is NetworkVP_vecnet.VectorNetwork's; this module states the layer list, the initial weights and what
ga3c_dmlp_create and ga3c_dmlp_evaluate take.
"""
import numpy as np

from Config import Config
from NetworkVP_vecnet import DeviceActors, VectorNetwork
import _native as nat

HEADS = ("logits_v", "logits_p")
# what ga3c_dmlp_actors_get names, per environment: dtype and elements ("batch_*": rows of the last step's batch instead)
ACTOR_FIELDS = {"phys": (np.float64, "S"), "elapsed": (np.int32, 1), "time_count": (np.int32, 1), "started": (np.int32, 1),
                "draws": (np.uint64, 1), "obs": (np.float32, "S"), "p": (np.float32, "A"), "v": (np.float32, 1),
                "u": (np.float64, 1), "action": (np.int32, 1), "reward": (np.float64, 1), "done": (np.int32, 1),
                "cut": (np.int32, 1), "rollout_len": (np.int32, 1),
                "batch_x": (np.float32, "S"), "batch_y_r": (np.float32, 1), "batch_a": (np.float32, "A")}
INIT = 0.3                  # dense_layer's U(-0.3, 0.3), weights and biases alike (NetworkVP.py:194-204)
STACKS = ("fork", "chained")


def _layers(layers=None):
    layers = tuple(int(w) for w in (Config.DENSE_LAYERS if layers is None else layers))
    if not 1 <= len(layers) <= 8 or any(not 1 <= w <= 256 for w in layers):
        raise ValueError("DENSE_LAYERS=%r: 1 to 8 widths of 1 to 256" % (layers,))
    return layers


def _stack(stack=None):
    stack = Config.DENSE_STACK if stack is None else stack
    if stack not in STACKS:
        raise ValueError("DENSE_STACK=%r: 'fork' or 'chained'" % (stack,))
    return stack


def param_order(layers=None):
    names = ["dense1_%d_p" % (i + 1) for i in range(len(_layers(layers)))] + list(HEADS)
    return tuple("%s/%s" % (layer, wb) for layer in names for wb in ("w", "b"))


def param_shapes(state_dim, num_actions, layers=None, stack=None):
    layers, chained = _layers(layers), _stack(stack) == "chained"
    shapes, fan_in = {}, int(state_dim)
    for i, width in enumerate(layers):
        name = "dense1_%d_p" % (i + 1)
        shapes[name + "/w"], shapes[name + "/b"] = (fan_in, width), (width,)
        if chained:
            fan_in = width
    for name, width in zip(HEADS, (1, int(num_actions))):
        shapes[name + "/w"], shapes[name + "/b"] = (layers[-1], width), (width,)
    return shapes


def dead_params(layers=None, stack=None):
    """The variables nothing reads: every dense layer but the last under DENSE_STACK = 'fork'."""
    layers = _layers(layers)
    if _stack(stack) == "chained":
        return ()
    return tuple("dense1_%d_p/%s" % (i + 1, wb) for i in range(len(layers) - 1) for wb in ("w", "b"))


def initial_arena(state_dim, num_actions, seed, layers=None, stack=None):
    """U(-0.3, 0.3) for every variable, the dead ones included, drawn from one PCG64(seed) stream in variable order."""
    rng = np.random.Generator(np.random.PCG64(seed))
    shapes = param_shapes(state_dim, num_actions, layers, stack)
    return np.concatenate([rng.uniform(-INIT, INIT, size=shapes[k]).astype(np.float32).ravel() for k in param_order(layers)])


class Network(DeviceActors, VectorNetwork):
    PREFIX = "ga3c_dmlp"
    LOGITS_PER_ACTION = 1
    ACTIVATION_TAGS = ("activation_lastdense",)   # NetworkVP_discrate.py:132-146; the dead variables get histograms too
    DUAL_RMSPROP_REFUSAL = "DUAL_RMSPROP with the discrete vector-state network is not supported"
    ACTOR_FIELDS = ACTOR_FIELDS   # device actors (Config.DEVICE_AGENTS): ga3c_dmlp_actors_*, CartPole-v0
    ACTOR_SCALARS = {"batch_rows": np.int32}
    ACTOR_ROWS = dict.fromkeys(("batch_x", "batch_y_r", "batch_a"), "batch_rows")

    def _config(self):
        self.layers, self.stack = _layers(), _stack()
        self.ACTIVATION_WIDTHS = (self.layers[-1],)
        cfg = nat.DmlpConfig()
        cfg.num_layers = len(self.layers)
        for i, width in enumerate(self.layers):
            cfg.widths[i] = width
        cfg.chained = int(self.stack == "chained")
        cfg.flags = (nat.FLAG_LOG_SOFTMAX if Config.USE_LOG_SOFTMAX else 0) | (nat.FLAG_GRAD_CLIP if Config.USE_GRAD_CLIP else 0)
        cfg.log_epsilon = Config.LOG_EPSILON
        cfg.min_policy = Config.MIN_POLICY
        return cfg

    def _variables(self):
        self.dead = dead_params(self.layers, self.stack)
        return (param_order(self.layers), param_shapes(self.S, self.num_actions, self.layers, self.stack),
                initial_arena(self.S, self.num_actions, Config.RANDOM_SEED, self.layers, self.stack))
