"""Network for vector-state games with a discrete action space (Config.GAME = 'CartPole-v0') -- the reference's third
network class (ga3c/NetworkVP_discrate.py:39-146; the module name is the reference's, sic), backed by the ga3c_dmlp handle
of libga3c_hip.so.

    x[B,S] -> dense1_<i>_p (Config.DENSE_LAYERS[i - 1] units, sigmoid), i = 1..L -> logits_v (1) and logits_p (A) -> softmax

Config.DENSE_STACK = 'fork' builds the layers as the reference does (:52-56): every one of them reads x and only the last
reaches the heads, so dense1_1_p .. dense1_<L-1>_p are variables that nothing reads -- created, initialised, saved and
histogrammed, never trained.  'chained' feeds layer i - 1 into layer i.

Same interface as NetworkVP_vector.Network.  It has no frame front-end, no state cache and no data-parallel or Hogwild
training: Server refuses those settings with this network.
"""
import ctypes as C
import glob
import os
import re
import threading

import numpy as np

from Config import Config
from NetworkVP import _device_ordinal, histogram_proto
import _native as nat

HEADS = ("logits_v", "logits_p")
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


class Network:
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
        if Config.DUAL_RMSPROP:
            raise ValueError("DUAL_RMSPROP with the discrete vector-state network is not supported")
        if max_batch is None:
            max_batch = max(Config.PREDICTION_BATCH_SIZE,
                            Config.TRAIN_ROWS_MAX or (Config.TRAINING_MIN_BATCH_SIZE + Config.TIME_MAX + 1))
        self.max_batch = int(max_batch)
        self._lib = nat.hip_lib()
        self.layers, self.stack = _layers(), _stack()
        cfg = nat.DmlpConfig()
        cfg.device = _device_ordinal(device)
        cfg.state_dim = self.S
        cfg.num_actions = self.num_actions
        cfg.max_batch = self.max_batch
        cfg.num_layers = len(self.layers)
        for i, width in enumerate(self.layers):
            cfg.widths[i] = width
        cfg.chained = int(self.stack == "chained")
        cfg.flags = (nat.FLAG_LOG_SOFTMAX if Config.USE_LOG_SOFTMAX else 0) | (nat.FLAG_GRAD_CLIP if Config.USE_GRAD_CLIP else 0)
        cfg.log_epsilon = Config.LOG_EPSILON
        cfg.min_policy = Config.MIN_POLICY
        cfg.rmsprop_decay = Config.RMSPROP_DECAY
        cfg.rmsprop_momentum = Config.RMSPROP_MOMENTUM
        cfg.rmsprop_epsilon = Config.RMSPROP_EPSILON
        cfg.grad_clip_norm = Config.GRAD_CLIP_NORM
        # the pipelined predictor loop holds two predictions per thread; the dynamic adjustment may add threads
        cfg.predict_lanes = int(predict_lanes or 2 * max(Config.PREDICTORS, 4 if Config.DYNAMIC_SETTINGS else 1) + 2)
        handle = C.c_void_p()
        nat.check(self._lib.ga3c_dmlp_create(C.byref(cfg), C.byref(handle)), "ga3c_dmlp_create")
        self._h = handle
        n = C.c_int64()
        nat.check(self._lib.ga3c_dmlp_param_count(self._h, C.byref(n)))
        self.param_count = n.value
        self.param_order = param_order(self.layers)
        self.dead = dead_params(self.layers, self.stack)
        self._offsets, off = {}, 0
        for name in self.param_order:
            size = int(np.prod(param_shapes(self.S, self.num_actions, self.layers, self.stack)[name]))
            self._offsets[name] = (off, size)
            off += size
        assert off == self.param_count
        self.set_arena(0, initial_arena(self.S, self.num_actions, Config.RANDOM_SEED, self.layers, self.stack))
        self._log_lock = threading.Lock()
        self.last_losses = None

    def close(self):
        if getattr(self, "_h", None):
            self._lib.ga3c_dmlp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- arenas: 0 weights, 1 / 2 RMSProp `ms` / `mom`, 3 last gradient -------------------------
    def get_arena(self, which):
        out = np.empty(self.param_count, dtype=np.float32)
        nat.check(self._lib.ga3c_dmlp_get_arena(self._h, which, nat.ptr(out), out.size), "ga3c_dmlp_get_arena")
        return out

    def set_arena(self, which, flat):
        flat = nat.as_f32(flat).ravel()
        nat.check(self._lib.ga3c_dmlp_set_arena(self._h, which, nat.ptr(flat), flat.size), "ga3c_dmlp_set_arena")

    def get_global_step(self):
        s = C.c_int64()
        nat.check(self._lib.ga3c_dmlp_get_step(self._h, C.byref(s)))
        return s.value

    def get_variables_names(self):
        n = self._lib.ga3c_dmlp_num_params(self._h)
        return [self._lib.ga3c_dmlp_param_name(self._h, i).decode() + ":0" for i in range(n)]

    def _param_info(self, name):
        off, count, ndim = C.c_int64(), C.c_int64(), C.c_int32()
        shape = (C.c_int64 * 4)()
        nat.check(self._lib.ga3c_dmlp_param_info(self._h, name.encode(), C.byref(off), C.byref(count), C.byref(ndim), shape),
                  "ga3c_dmlp_param_info")
        return off.value, count.value, tuple(shape[d] for d in range(ndim.value))

    def get_variable_value(self, name, which=0):
        _, count, shape = self._param_info(name)
        out = np.empty(count, dtype=np.float32)
        nat.check(self._lib.ga3c_dmlp_get_param(self._h, name.encode(), which, nat.ptr(out), count), "ga3c_dmlp_get_param")
        return out.reshape(shape)

    def set_variable_value(self, name, value, which=0):
        flat = nat.as_f32(value).ravel()
        nat.check(self._lib.ga3c_dmlp_set_param(self._h, name.encode(), which, nat.ptr(flat), flat.size), "ga3c_dmlp_set_param")

    # ---- inference ---------------------------------------------------------------------------
    def _rows(self, x):
        x = nat.as_f32(x).reshape(-1, self.S)
        return x, int(x.shape[0])

    def predict_p_v_logits(self, x):
        x, b = self._rows(x)
        p = np.empty((b, self.num_actions), np.float32)
        v = np.empty(b, np.float32)
        z = np.empty((b, self.num_actions), np.float32)
        nat.check(self._lib.ga3c_dmlp_predict(self._h, nat.ptr(x), b, nat.ptr(p), nat.ptr(v), nat.ptr(z)), "ga3c_dmlp_predict")
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
    def register_transport(self, transport):
        nat.check(self._lib.ga3c_dmlp_register_host(self._h, C.c_void_p(transport.base), transport.nbytes),
                  "ga3c_dmlp_register_host")

    def unregister_transport(self):
        nat.check(self._lib.ga3c_dmlp_unregister_host(self._h), "ga3c_dmlp_unregister_host")

    def gather_entry(self):
        """(address of ga3c_dmlp_predict_gather, handle, u8 = 0) for the native predictor loop (ga3c_pq_serve)."""
        return C.cast(self._lib.ga3c_dmlp_predict_gather, C.c_void_p).value, self._h, 0

    def gather_entries_pipelined(self):
        """(addresses of ga3c_dmlp_predict_gather_begin / _end, handle, u8 = 0) for ga3c_pq_serve_pipelined."""
        return (C.cast(self._lib.ga3c_dmlp_predict_gather_begin, C.c_void_p).value,
                C.cast(self._lib.ga3c_dmlp_predict_gather_end, C.c_void_p).value, self._h, 0)

    def predict_offsets(self, offsets):
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        b = offsets.size
        p = np.empty((b, self.num_actions), np.float32)
        v = np.empty(b, np.float32)
        nat.check(self._lib.ga3c_dmlp_predict_gather(self._h, nat.ptr(offsets, nat.i64p), b, 0, nat.ptr(p), nat.ptr(v), None),
                  "ga3c_dmlp_predict_gather")
        return [p, v]

    def train_offsets(self, offsets, y_r, a):
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        y, a = nat.as_f32(y_r), nat.as_f32(a)
        losses = np.empty(3, np.float32)
        nat.check(self._lib.ga3c_dmlp_train_gather(self._h, nat.ptr(offsets, nat.i64p), 0, nat.ptr(y), nat.ptr(a), offsets.size,
                                                  float(self.learning_rate), float(self.beta), nat.ptr(losses)),
                  "ga3c_dmlp_train_gather")
        self.last_losses = losses

    # ---- training ----------------------------------------------------------------------------
    def train(self, x, y_r, a, x2=None, done=None, trainer_id=0):
        """x2, done and trainer_id are accepted and ignored, as in NetworkVP.py:254-257."""
        x, b = self._rows(x)
        y, a = nat.as_f32(y_r), nat.as_f32(a)
        losses = np.empty(3, np.float32)
        nat.check(self._lib.ga3c_dmlp_train(self._h, nat.ptr(x), nat.ptr(y), nat.ptr(a), b, float(self.learning_rate),
                                           float(self.beta), nat.ptr(losses)), "ga3c_dmlp_train")
        self.last_losses = losses

    def compute_grads(self, x, y_r, a):
        x, b = self._rows(x)
        y, a = nat.as_f32(y_r), nat.as_f32(a)
        losses = np.empty(3, np.float32)
        nat.check(self._lib.ga3c_dmlp_compute_grads(self._h, nat.ptr(x), nat.ptr(y), nat.ptr(a), b, float(self.beta),
                                                   nat.ptr(losses)), "ga3c_dmlp_compute_grads")
        return losses

    def apply_grads(self):
        nat.check(self._lib.ga3c_dmlp_apply_grads(self._h, float(self.learning_rate)), "ga3c_dmlp_apply_grads")

    def fetch(self, name, count):
        out = np.empty(int(count), np.float32)
        nat.check(self._lib.ga3c_dmlp_fetch(self._h, name.encode(), nat.ptr(out), out.size), "ga3c_dmlp_fetch")
        return out

    def upload(self, x, y_r, a):
        x, b = self._rows(x)
        y, a = nat.as_f32(y_r), nat.as_f32(a)
        nat.check(self._lib.ga3c_dmlp_upload(self._h, nat.ptr(x), nat.ptr(y), nat.ptr(a), b), "ga3c_dmlp_upload")

    def time_resident(self, mode, batch, iters):
        """Milliseconds of `iters` resident steps (mode 0 predict, 1 train) on the first `batch` uploaded rows."""
        ms = C.c_float()
        nat.check(self._lib.ga3c_dmlp_time_resident(self._h, int(mode), int(batch), int(iters), float(self.learning_rate),
                                                   float(self.beta), C.byref(ms)), "ga3c_dmlp_time_resident")
        return ms.value

    # ---- logging / checkpoints -----------------------------------------------------------------
    def evaluate(self, x, y_r, a, offsets=None):
        """Forward + loss of the batch on the current weights, no update (sess.run(summary_op), NetworkVP.py:259-265).
        -> (losses[3], lastdense[B,w_L], v[B], p[B,A])."""
        y, a = nat.as_f32(y_r), nat.as_f32(a)
        b = int(y.shape[0])
        losses = np.empty(3, np.float32)
        last = np.empty((b, self.layers[-1]), np.float32)
        v, p = np.empty(b, np.float32), np.empty((b, self.num_actions), np.float32)
        if offsets is not None:
            offsets = np.ascontiguousarray(offsets, dtype=np.int64)
            xs, os_ = None, nat.ptr(offsets, nat.i64p)
        else:
            x, _ = self._rows(x)
            xs, os_ = nat.ptr(x), None
        nat.check(self._lib.ga3c_dmlp_evaluate(self._h, xs, os_, nat.ptr(y), nat.ptr(a), b, float(self.beta), nat.ptr(losses),
                                               nat.ptr(last), nat.ptr(v), nat.ptr(p)), "ga3c_dmlp_evaluate")
        return losses, last, v, p

    def log(self, x, y_r, a, training_step, feed_dict=None, offsets=None, frames=None):
        """The reference's summary_op on the batch it is given (NetworkVP_discrate.py:132-146): the six scalars appended to
        logs/<model>/scalars.csv, and the histograms (one per trainable variable -- the dead ones too, tf.trainable_variables()
        lists them --, activation_lastdense, activation_v, activation_p) in logs/<model>/histograms_%08d.npz with
        HistogramProto's fields."""
        if frames is not None:
            raise ValueError("the vector-state network keeps no states on the device")
        losses, last, v, p = self.evaluate(x, y_r, a, offsets=offsets)
        c1, c2, cv = (float(t) for t in losses)
        theta = self.get_arena(0)
        hist = {}
        for name in self.param_order:
            off, size = self._offsets[name]
            hist["weights_%s:0" % name] = histogram_proto(theta[off:off + size])
        for tag, val in (("activation_lastdense", last), ("activation_v", v), ("activation_p", p)):
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

    def _checkpoint_filename(self, episode):
        return 'checkpoints/%s_%08d' % (self.model_name, episode)

    def save(self, episode):
        os.makedirs("checkpoints", exist_ok=True)
        nat.check(self._lib.ga3c_dmlp_save(self._h, (self._checkpoint_filename(episode) + ".npz").encode()), "ga3c_dmlp_save")

    def load(self):
        if Config.LOAD_EPISODE > 0:
            filename = self._checkpoint_filename(Config.LOAD_EPISODE) + ".npz"
        else:
            found = sorted(glob.glob('checkpoints/%s_????????.npz' % self.model_name))
            if not found:
                raise FileNotFoundError("no checkpoint for %s" % self.model_name)
            filename = found[-1]
        nat.check(self._lib.ga3c_dmlp_load(self._h, filename.encode()), "ga3c_dmlp_load")
        return int(re.split(r'/|_|\.', filename[:-4])[2])
