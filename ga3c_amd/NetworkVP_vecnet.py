"""What the vector-state networks share on the Python side (NetworkVP_vector.Network, NetworkVP_discrate.Network): the
handle of libga3c_hip.so behind them has one host implementation (csrc/ga3c_vecnet.hpp) and one entry
list under two prefixes, so every call but create and evaluate is made here or in NativeHandle.py, whose classes hold the
part that the image network (ParamHandle) and NetworkDDPG.Network (NativeHandle) share as well.

Same interface as NetworkVP.Network where Server, ThreadPredictor and ThreadTrainer use it (predict_p_and_v, train, log,
save, load, get_global_step, get_variables_names, get_variable_value, and the zero-copy entries).  There is no frame
front-end, no state cache and no data-parallel or Hogwild training: Server refuses those settings with these networks.

A subclass states PREFIX, LOGITS_PER_ACTION, ACTIVATION_WIDTHS / ACTIVATION_TAGS (or its own evaluate), DUAL_RMSPROP_REFUSAL
(None where its handle takes the flag), _config() and _variables().  DeviceActors is the mixin of the networks whose handles
step their own environments (Config.DEVICE_AGENTS), NetworkDDPG.Network among them: the actors_* methods over
<PREFIX>_actors_*.
"""
import ctypes as C
import os
import threading

import numpy as np

from Config import Config
from NativeHandle import NativeHandle, ParamHandle  # noqa: F401  (NativeHandle: NetworkDDPG imports it from here)
from NetworkVP import _device_ordinal, histogram_proto
import _native as nat


class VectorNetwork(ParamHandle):
    LOGITS_PER_ACTION = None
    ACTIVATION_WIDTHS = ()        # the activation outputs of <PREFIX>_evaluate, and the tags log() gives them
    ACTIVATION_TAGS = ()
    DUAL_RMSPROP_REFUSAL = None

    def _config(self):
        """-> the network's config struct with the fields of its own filled, flags among them."""
        raise NotImplementedError

    def _variables(self):
        """-> (variable names in arena order, {name: shape}, the initial arena)."""
        raise NotImplementedError

    def __init__(self, device, model_name, num_actions, state_dim, max_batch=None, predict_lanes=None):
        self.device = device
        self.model_name = model_name
        self.num_actions = int(num_actions)
        self.state_dim = tuple(state_dim) if np.ndim(state_dim) else (int(state_dim),)
        if len(self.state_dim) != 1:
            raise ValueError("state_dim %r is not a vector" % (state_dim,))
        self.S = int(self.state_dim[0])
        self.learning_rate = Config.LEARNING_RATE_START
        self.beta = Config.BETA_START
        if Config.DUAL_RMSPROP and self.DUAL_RMSPROP_REFUSAL:
            raise ValueError(self.DUAL_RMSPROP_REFUSAL)
        if max_batch is None:
            max_batch = max(Config.PREDICTION_BATCH_SIZE,
                            Config.TRAIN_ROWS_MAX or (Config.TRAINING_MIN_BATCH_SIZE + Config.TIME_MAX + 1))
        self.max_batch = int(max_batch)
        self._lib = nat.hip_lib()
        cfg = self._config()
        cfg.device = _device_ordinal(device)
        cfg.state_dim = self.S
        cfg.num_actions = self.num_actions
        cfg.max_batch = self.max_batch
        cfg.rmsprop_decay = Config.RMSPROP_DECAY
        cfg.rmsprop_momentum = Config.RMSPROP_MOMENTUM
        cfg.rmsprop_epsilon = Config.RMSPROP_EPSILON
        cfg.grad_clip_norm = Config.GRAD_CLIP_NORM
        # the pipelined predictor loop holds two predictions per thread; the dynamic adjustment may add threads
        cfg.predict_lanes = int(predict_lanes or 2 * max(Config.PREDICTORS, 4 if Config.DYNAMIC_SETTINGS else 1) + 2)
        handle = C.c_void_p()
        nat.check(self._fn("create")(C.byref(cfg), C.byref(handle)), self.PREFIX + "_create")
        self._h = handle
        n = C.c_int64()
        nat.check(self._fn("param_count")(self._h, C.byref(n)))
        self.param_count = n.value
        self.param_order, shapes, theta = self._variables()
        self._offsets, off = {}, 0
        for name in self.param_order:
            size = int(np.prod(shapes[name]))
            self._offsets[name] = (off, size)
            off += size
        assert off == self.param_count
        self.set_arena(0, theta)
        self._log_lock = threading.Lock()
        self.last_losses = None

    # ---- inference ---------------------------------------------------------------------------
    def predict_p_v_logits(self, x):
        x, b = self._rows(x)
        p = np.empty((b, self.num_actions), np.float32)
        v = np.empty(b, np.float32)
        z = np.empty((b, self.LOGITS_PER_ACTION * self.num_actions), np.float32)
        self._call("predict", nat.ptr(x), b, nat.ptr(p), nat.ptr(v), nat.ptr(z))
        return p, v, z

    def predict_p_and_v(self, x):
        p, v, _ = self.predict_p_v_logits(x)
        return [p, v]

    def predict_p(self, x):
        return self.predict_p_and_v(x)[0]

    def predict_v(self, x):
        return self.predict_p_and_v(x)[1]

    def predict_single(self, x):
        return self.predict_p(x[None, :])[0]

    # ---- zero-copy intake from the shared-memory transport (rows of 4 S bytes) -------------------
    def predict_offsets(self, offsets):
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        b = offsets.size
        p = np.empty((b, self.num_actions), np.float32)
        v = np.empty(b, np.float32)
        self._call("predict_gather", nat.ptr(offsets, nat.i64p), b, 0, nat.ptr(p), nat.ptr(v), None)
        return [p, v]

    def train_offsets(self, offsets, y_r, a):
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        y, a = nat.as_f32(y_r), nat.as_f32(a)
        losses = np.empty(3, np.float32)
        self._call("train_gather", nat.ptr(offsets, nat.i64p), 0, nat.ptr(y), nat.ptr(a), offsets.size,
                   float(self.learning_rate), float(self.beta), nat.ptr(losses))
        self.last_losses = losses

    # ---- training ----------------------------------------------------------------------------
    def train(self, x, y_r, a, x2=None, done=None, trainer_id=0):
        """x2, done and trainer_id are accepted and ignored, as in NetworkVP.py:254-257."""
        x, b = self._rows(x)
        y, a = nat.as_f32(y_r), nat.as_f32(a)
        losses = np.empty(3, np.float32)
        self._call("train", nat.ptr(x), nat.ptr(y), nat.ptr(a), b, float(self.learning_rate), float(self.beta),
                   nat.ptr(losses))
        self.last_losses = losses

    def compute_grads(self, x, y_r, a):
        x, b = self._rows(x)
        y, a = nat.as_f32(y_r), nat.as_f32(a)
        losses = np.empty(3, np.float32)
        self._call("compute_grads", nat.ptr(x), nat.ptr(y), nat.ptr(a), b, float(self.beta), nat.ptr(losses))
        return losses

    def apply_grads(self):
        self._call("apply_grads", float(self.learning_rate))

    def upload(self, x, y_r, a):
        x, b = self._rows(x)
        y, a = nat.as_f32(y_r), nat.as_f32(a)
        self._call("upload", nat.ptr(x), nat.ptr(y), nat.ptr(a), b)

    def time_resident(self, mode, batch, iters):
        """Milliseconds of `iters` resident steps (mode 0 predict, 1 train) on the first `batch` uploaded rows."""
        ms = C.c_float()
        self._call("time_resident", int(mode), int(batch), int(iters), float(self.learning_rate), float(self.beta),
                   C.byref(ms))
        return ms.value

    # ---- logging / checkpoints -----------------------------------------------------------------
    def evaluate(self, x, y_r, a, offsets=None):
        """Forward + loss of the batch on the current weights, no update (sess.run(summary_op), NetworkVP.py:259-265).
        -> (losses[3], one [B, w] array per ACTIVATION_WIDTHS, v[B], p[B,A])."""
        y, a = nat.as_f32(y_r), nat.as_f32(a)
        b = int(y.shape[0])
        losses = np.empty(3, np.float32)
        acts = [np.empty((b, w), np.float32) for w in self.ACTIVATION_WIDTHS]
        v, p = np.empty(b, np.float32), np.empty((b, self.num_actions), np.float32)
        if offsets is not None:
            offsets = np.ascontiguousarray(offsets, dtype=np.int64)
            xs, os_ = None, nat.ptr(offsets, nat.i64p)
        else:
            x, _ = self._rows(x)
            xs, os_ = nat.ptr(x), None
        self._call("evaluate", xs, os_, nat.ptr(y), nat.ptr(a), b, float(self.beta), nat.ptr(losses),
                   *[nat.ptr(t) for t in acts + [v, p]])
        return (losses, *acts, v, p)

    def log(self, x, y_r, a, training_step, feed_dict=None, offsets=None, frames=None):
        """The reference's summary_op on the batch it is given: the six scalars appended to logs/<model>/scalars.csv, and the
        histograms (one per trainable variable, then ACTIVATION_TAGS, activation_v, activation_p) in
        logs/<model>/histograms_%08d.npz with HistogramProto's fields."""
        if frames is not None:
            raise ValueError("the vector-state network keeps no states on the device")
        losses, *acts = self.evaluate(x, y_r, a, offsets=offsets)
        c1, c2, cv = (float(t) for t in losses)
        theta = self.get_arena(0)
        hist = {}
        for name in self.param_order:
            off, size = self._offsets[name]
            hist["weights_%s:0" % name] = histogram_proto(theta[off:off + size])
        for tag, val in zip(self.ACTIVATION_TAGS + ("activation_v", "activation_p"), acts):
            hist[tag] = histogram_proto(val)
        out = {"%s/%s" % (tag, field): value for tag, h in hist.items() for field, value in h.items()}
        os.makedirs("logs/%s" % self.model_name, exist_ok=True)
        with self._log_lock:
            with open("logs/%s/scalars.csv" % self.model_name, "a") as f:
                f.write("%d,%.8g,%.8g,%.8g,%.8g,%.8g,%.8g\n" % (training_step, c1, c2, -(c1 + c2), cv,
                                                                self.learning_rate, self.beta))
            tmp = "logs/%s/histograms_%08d.tmp.npz" % (self.model_name, training_step)
            np.savez(tmp, **out)
            os.replace(tmp, "logs/%s/histograms_%08d.npz" % (self.model_name, training_step))
        return losses


class DeviceActors:
    """Config.DEVICE_AGENTS: the <PREFIX>_actors_* entries of a network whose handle steps its
    environments itself (csrc/ga3c_actors.hpp).  Mixed into NetworkVP_discrate.Network (CartPole-v0), NetworkVP_vector.Network
    (Pendulum-v0) and NetworkDDPG.Network (Pendulum-v0 into a replay ring; its own actors_create and actors_run).  Each states
    what <PREFIX>_actors_get names:
      ACTOR_FIELDS   {name: (dtype, elements per row -- a number, "S" or "A")}, one row per environment unless ACTOR_ROWS says otherwise;
      ACTOR_SCALARS  {name: dtype} of the handle's single values;
      ACTOR_ROWS     {field name: the scalar that is its row count}."""
    ACTOR_FIELDS = {}
    ACTOR_SCALARS = {}
    ACTOR_ROWS = {}

    def actors_create(self, n, time_max=None, discount=None, seed=None):
        self._call("actors_create", int(n), int(Config.TIME_MAX if time_max is None else time_max),
                   float(Config.DISCOUNT if discount is None else discount), int(Config.RANDOM_SEED if seed is None else seed))
        self.num_actors = int(n)

    def actors_destroy(self):
        self._call("actors_destroy")

    def actors_run(self, steps, train=True):
        """`steps` actor steps at the model's learning_rate and beta -> (agent steps, train calls, rows trained, episodes
        finished)."""
        stats = np.zeros(4, np.int64)
        self._call("actors_run", int(steps), float(self.learning_rate), float(self.beta), int(bool(train)),
                   nat.ptr(stats, nat.i64p))
        return tuple(int(t) for t in stats)

    def actors_episodes(self, max_count=4096):
        """The finished episodes not yet taken, oldest first -> [(total_reward, total_length)]."""
        out = []
        reward, length, count = np.empty(max_count, np.float64), np.empty(max_count, np.int64), C.c_int32()
        while True:
            self._call("actors_episodes", nat.ptr(reward, nat.f64p), nat.ptr(length, nat.i64p), max_count, C.byref(count))
            out += [(float(reward[i]), int(length[i])) for i in range(count.value)]
            if count.value < max_count:
                return out

    def actors_get(self, name):
        if name in self.ACTOR_SCALARS:
            out = np.zeros(1, self.ACTOR_SCALARS[name])
            self._call("actors_get", name.encode(), out.ctypes.data_as(C.c_void_p), out.nbytes)
            return int(out[0])
        dtype, width = self.ACTOR_FIELDS[name]
        vector = width != 1                         # "S" / "A" fields are [rows, width] whatever the width, the others [rows]
        width = {"S": self.S, "A": self.num_actions}.get(width, width)
        rows = self.actors_get(self.ACTOR_ROWS[name]) if name in self.ACTOR_ROWS else self.num_actors
        out = np.zeros((rows, width) if vector else (rows,), dtype)
        self._call("actors_get", name.encode(), out.ctypes.data_as(C.c_void_p), out.nbytes)
        return out

    def actors_set(self, name, value):
        dtype = self.ACTOR_SCALARS[name] if name in self.ACTOR_SCALARS else self.ACTOR_FIELDS[name][0]
        value = np.ascontiguousarray(value, dtype=dtype)
        self._call("actors_set", name.encode(), value.ctypes.data_as(C.c_void_p), value.nbytes)
