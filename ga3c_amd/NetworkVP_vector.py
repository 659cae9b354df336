"""Network for vector-state games (Config.GAME = 'Pendulum-v0') -- the network the reference fork itself trains
(/root/reference/ga3c/NetworkVP.py:67-105,164-210), backed by the ga3c_mlp handle of libga3c_hip.so.

    x[B,S] -> dense11_p (4) -> dense12_p (256) -> dense13_p (256) -> dense14_p (100, sigmoid) -> dense1 (64, sigmoid)
           -> logits_v (1) and the angle-output head logits_p/out_x, out_y (A each, sigmoid): p = atan2(Y, X) / pi

Same interface as NetworkVP.Network where Server, ThreadPredictor and ThreadTrainer use it (predict_p_and_v, train, log,
save, load, get_global_step, get_variables_names, get_variable_value, and the zero-copy entries).  It has no frame
front-end, no state cache and no data-parallel or Hogwild training: Server refuses those settings with this network.
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

TRUNK = (("dense11_p", 4), ("dense12_p", 256), ("dense13_p", 256), ("dense14_p", 100), ("dense1", 64))
HEADS = ("logits_v", "logits_p/out_x", "logits_p/out_y")
INIT = 0.3                  # dense_layer's U(-0.3, 0.3), weights and biases alike (NetworkVP.py:194-204)


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
            raise ValueError("DUAL_RMSPROP with the continuous head is not supported")
        if max_batch is None:
            max_batch = max(Config.PREDICTION_BATCH_SIZE,
                            Config.TRAIN_ROWS_MAX or (Config.TRAINING_MIN_BATCH_SIZE + Config.TIME_MAX + 1))
        self.max_batch = int(max_batch)
        self._lib = nat.hip_lib()
        cfg = nat.MlpConfig()
        cfg.device = _device_ordinal(device)
        cfg.state_dim = self.S
        cfg.num_actions = self.num_actions
        cfg.max_batch = self.max_batch
        cfg.flags = nat.FLAG_CONTINUOUS | (nat.FLAG_GRAD_CLIP if Config.USE_GRAD_CLIP else 0)
        cfg.rmsprop_decay = Config.RMSPROP_DECAY
        cfg.rmsprop_momentum = Config.RMSPROP_MOMENTUM
        cfg.rmsprop_epsilon = Config.RMSPROP_EPSILON
        cfg.grad_clip_norm = Config.GRAD_CLIP_NORM
        # the pipelined predictor loop holds two predictions per thread; the dynamic adjustment may add threads
        cfg.predict_lanes = int(predict_lanes or 2 * max(Config.PREDICTORS, 4 if Config.DYNAMIC_SETTINGS else 1) + 2)
        handle = C.c_void_p()
        nat.check(self._lib.ga3c_mlp_create(C.byref(cfg), C.byref(handle)), "ga3c_mlp_create")
        self._h = handle
        n = C.c_int64()
        nat.check(self._lib.ga3c_mlp_param_count(self._h, C.byref(n)))
        self.param_count = n.value
        self.param_order = param_order()
        self._offsets, off = {}, 0
        for name in self.param_order:
            size = int(np.prod(param_shapes(self.S, self.num_actions)[name]))
            self._offsets[name] = (off, size)
            off += size
        assert off == self.param_count
        self.set_arena(0, initial_arena(self.S, self.num_actions, Config.RANDOM_SEED))
        self._log_lock = threading.Lock()
        self.last_losses = None

    def close(self):
        if getattr(self, "_h", None):
            self._lib.ga3c_mlp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- arenas: 0 weights, 1 / 2 RMSProp `ms` / `mom`, 3 last gradient -------------------------
    def get_arena(self, which):
        out = np.empty(self.param_count, dtype=np.float32)
        nat.check(self._lib.ga3c_mlp_get_arena(self._h, which, nat.ptr(out), out.size), "ga3c_mlp_get_arena")
        return out

    def set_arena(self, which, flat):
        flat = nat.as_f32(flat).ravel()
        nat.check(self._lib.ga3c_mlp_set_arena(self._h, which, nat.ptr(flat), flat.size), "ga3c_mlp_set_arena")

    def get_global_step(self):
        s = C.c_int64()
        nat.check(self._lib.ga3c_mlp_get_step(self._h, C.byref(s)))
        return s.value

    def get_variables_names(self):
        n = self._lib.ga3c_mlp_num_params(self._h)
        return [self._lib.ga3c_mlp_param_name(self._h, i).decode() + ":0" for i in range(n)]

    def _param_info(self, name):
        off, count, ndim = C.c_int64(), C.c_int64(), C.c_int32()
        shape = (C.c_int64 * 4)()
        nat.check(self._lib.ga3c_mlp_param_info(self._h, name.encode(), C.byref(off), C.byref(count), C.byref(ndim), shape),
                  "ga3c_mlp_param_info")
        return off.value, count.value, tuple(shape[d] for d in range(ndim.value))

    def get_variable_value(self, name, which=0):
        _, count, shape = self._param_info(name)
        out = np.empty(count, dtype=np.float32)
        nat.check(self._lib.ga3c_mlp_get_param(self._h, name.encode(), which, nat.ptr(out), count), "ga3c_mlp_get_param")
        return out.reshape(shape)

    def set_variable_value(self, name, value, which=0):
        flat = nat.as_f32(value).ravel()
        nat.check(self._lib.ga3c_mlp_set_param(self._h, name.encode(), which, nat.ptr(flat), flat.size), "ga3c_mlp_set_param")

    # ---- inference ---------------------------------------------------------------------------
    def _rows(self, x):
        x = nat.as_f32(x).reshape(-1, self.S)
        return x, int(x.shape[0])

    def predict_p_v_logits(self, x):
        x, b = self._rows(x)
        p = np.empty((b, self.num_actions), np.float32)
        v = np.empty(b, np.float32)
        z = np.empty((b, 2 * self.num_actions), np.float32)
        nat.check(self._lib.ga3c_mlp_predict(self._h, nat.ptr(x), b, nat.ptr(p), nat.ptr(v), nat.ptr(z)), "ga3c_mlp_predict")
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
        nat.check(self._lib.ga3c_mlp_register_host(self._h, C.c_void_p(transport.base), transport.nbytes),
                  "ga3c_mlp_register_host")

    def unregister_transport(self):
        nat.check(self._lib.ga3c_mlp_unregister_host(self._h), "ga3c_mlp_unregister_host")

    def gather_entry(self):
        """(address of ga3c_mlp_predict_gather, handle, u8 = 0) for the native predictor loop (ga3c_pq_serve)."""
        return C.cast(self._lib.ga3c_mlp_predict_gather, C.c_void_p).value, self._h, 0

    def gather_entries_pipelined(self):
        """(addresses of ga3c_mlp_predict_gather_begin / _end, handle, u8 = 0) for ga3c_pq_serve_pipelined."""
        return (C.cast(self._lib.ga3c_mlp_predict_gather_begin, C.c_void_p).value,
                C.cast(self._lib.ga3c_mlp_predict_gather_end, C.c_void_p).value, self._h, 0)

    def predict_offsets(self, offsets):
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        b = offsets.size
        p = np.empty((b, self.num_actions), np.float32)
        v = np.empty(b, np.float32)
        nat.check(self._lib.ga3c_mlp_predict_gather(self._h, nat.ptr(offsets, nat.i64p), b, 0, nat.ptr(p), nat.ptr(v), None),
                  "ga3c_mlp_predict_gather")
        return [p, v]

    def train_offsets(self, offsets, y_r, a):
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        y, a = nat.as_f32(y_r), nat.as_f32(a)
        losses = np.empty(3, np.float32)
        nat.check(self._lib.ga3c_mlp_train_gather(self._h, nat.ptr(offsets, nat.i64p), 0, nat.ptr(y), nat.ptr(a), offsets.size,
                                                  float(self.learning_rate), float(self.beta), nat.ptr(losses)),
                  "ga3c_mlp_train_gather")
        self.last_losses = losses

    # ---- training ----------------------------------------------------------------------------
    def train(self, x, y_r, a, x2=None, done=None, trainer_id=0):
        """x2, done and trainer_id are accepted and ignored, as in NetworkVP.py:254-257."""
        x, b = self._rows(x)
        y, a = nat.as_f32(y_r), nat.as_f32(a)
        losses = np.empty(3, np.float32)
        nat.check(self._lib.ga3c_mlp_train(self._h, nat.ptr(x), nat.ptr(y), nat.ptr(a), b, float(self.learning_rate),
                                           float(self.beta), nat.ptr(losses)), "ga3c_mlp_train")
        self.last_losses = losses

    def compute_grads(self, x, y_r, a):
        x, b = self._rows(x)
        y, a = nat.as_f32(y_r), nat.as_f32(a)
        losses = np.empty(3, np.float32)
        nat.check(self._lib.ga3c_mlp_compute_grads(self._h, nat.ptr(x), nat.ptr(y), nat.ptr(a), b, float(self.beta),
                                                   nat.ptr(losses)), "ga3c_mlp_compute_grads")
        return losses

    def apply_grads(self):
        nat.check(self._lib.ga3c_mlp_apply_grads(self._h, float(self.learning_rate)), "ga3c_mlp_apply_grads")

    def fetch(self, name, count):
        out = np.empty(int(count), np.float32)
        nat.check(self._lib.ga3c_mlp_fetch(self._h, name.encode(), nat.ptr(out), out.size), "ga3c_mlp_fetch")
        return out

    def upload(self, x, y_r, a):
        x, b = self._rows(x)
        y, a = nat.as_f32(y_r), nat.as_f32(a)
        nat.check(self._lib.ga3c_mlp_upload(self._h, nat.ptr(x), nat.ptr(y), nat.ptr(a), b), "ga3c_mlp_upload")

    def time_resident(self, mode, batch, iters):
        """Milliseconds of `iters` resident steps (mode 0 predict, 1 train) on the first `batch` uploaded rows."""
        ms = C.c_float()
        nat.check(self._lib.ga3c_mlp_time_resident(self._h, int(mode), int(batch), int(iters), float(self.learning_rate),
                                                   float(self.beta), C.byref(ms)), "ga3c_mlp_time_resident")
        return ms.value

    # ---- logging / checkpoints -----------------------------------------------------------------
    def evaluate(self, x, y_r, a, offsets=None):
        """Forward + loss of the batch on the current weights, no update (sess.run(summary_op), NetworkVP.py:259-265).
        -> (losses[3], pd1[B,4], pd2[B,256], d1[B,64], v[B], p[B,A])."""
        y, a = nat.as_f32(y_r), nat.as_f32(a)
        b = int(y.shape[0])
        losses = np.empty(3, np.float32)
        pd1, pd2, d1 = np.empty((b, 4), np.float32), np.empty((b, 256), np.float32), np.empty((b, 64), np.float32)
        v, p = np.empty(b, np.float32), np.empty((b, self.num_actions), np.float32)
        if offsets is not None:
            offsets = np.ascontiguousarray(offsets, dtype=np.int64)
            xs, os_ = None, nat.ptr(offsets, nat.i64p)
        else:
            x, _ = self._rows(x)
            xs, os_ = nat.ptr(x), None
        nat.check(self._lib.ga3c_mlp_evaluate(self._h, xs, os_, nat.ptr(y), nat.ptr(a), b, float(self.beta), nat.ptr(losses),
                                              nat.ptr(pd1), nat.ptr(pd2), nat.ptr(d1), nat.ptr(v), nat.ptr(p)),
                  "ga3c_mlp_evaluate")
        return losses, pd1, pd2, d1, v, p

    def log(self, x, y_r, a, training_step, feed_dict=None, offsets=None, frames=None):
        """The reference's summary_op on the batch it is given (NetworkVP.py:150-170): the six scalars appended to
        logs/<model>/scalars.csv, and the histograms (one per trainable variable, activation_pd1, activation_pd2,
        activation_d2, activation_v, activation_p) in logs/<model>/histograms_%08d.npz with HistogramProto's fields."""
        if frames is not None:
            raise ValueError("the vector-state network keeps no states on the device")
        losses, pd1, pd2, d1, v, p = self.evaluate(x, y_r, a, offsets=offsets)
        c1, c2, cv = (float(t) for t in losses)
        theta = self.get_arena(0)
        hist = {}
        for name in self.param_order:
            off, size = self._offsets[name]
            hist["weights_%s:0" % name] = histogram_proto(theta[off:off + size])
        for tag, val in (("activation_pd1", pd1), ("activation_pd2", pd2), ("activation_d2", d1), ("activation_v", v),
                         ("activation_p", p)):
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
        nat.check(self._lib.ga3c_mlp_save(self._h, (self._checkpoint_filename(episode) + ".npz").encode()), "ga3c_mlp_save")

    def load(self):
        if Config.LOAD_EPISODE > 0:
            filename = self._checkpoint_filename(Config.LOAD_EPISODE) + ".npz"
        else:
            found = sorted(glob.glob('checkpoints/%s_????????.npz' % self.model_name))
            if not found:
                raise FileNotFoundError("no checkpoint for %s" % self.model_name)
            filename = found[-1]
        nat.check(self._lib.ga3c_mlp_load(self._h, filename.encode()), "ga3c_mlp_load")
        return int(re.split(r'/|_|\.', filename[:-4])[2])
