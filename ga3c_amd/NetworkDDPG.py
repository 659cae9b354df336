"""DDPG for vector-state games with continuous actions (Config.USE_DDPG) -- reference NetworkDDPG.py, backed by the
ga3c_ddpg handle of libga3c_hip.so.

    actor   x[B,S] -> actor_fc1 (400) -> actor_norm1 -> relu -> actor_fc2 (300) -> actor_norm2 -> relu -> actor_output (A, tanh)
    critic  x -> critic_fc1 (400) -> critic_norm1 -> relu = h;  q = critic_output(relu(h W_fc2 + a W_n2 + b_n2))

Same interface as NetworkVP.Network where Server, ThreadPredictor and ThreadTrainer use it.  The replay memory lives in
the handle (replay_add*, train_replay); the Ornstein-Uhlenbeck process too, because the native predictor loops call the
handle without the interpreter.  Under Config.PRIORITIZED_REPLAY the handle also keeps a priority per ring slot and draws a
step's rows itself (train_prioritized).  Under Config.DDPG_TWIN it has a second critic, critic2_*, and every
train-type call runs the twin step (twin_create).  Under Config.DDPG_NSTEP > 1 the device actors write n-step
returns into the ring and a discount per slot beside them (nstep_create).  Under Config.DDPG_DISTRIBUTIONAL the
critic's head has Config.DDPG_ATOMS outputs, a categorical distribution over fixed returns (dist_create).
eval_create attaches environments that the actor walks without noise from fixed start states, an episode per launch: how
good the actor is right now, with nothing of the training disturbed (Config.DEVICE_DDPG_EVAL_ENVS).
Under Config.DEVICE_DDPG_NOISE = 'per_env' every device actor has an Ornstein-Uhlenbeck process of its own, stepped in the predict
kernel (envnoise_create).  Under Config.DDPG_POPART the critic regresses on normalised targets and the handle has
two more variables, critic_popart/mu and /nu, the statistics that its output layer is rescaled with (popart_create).
Under a non-default Config.DEVICE_DDPG_ACTION_BOUND, _TIME_LIMIT, _RESET_OBSERVATION, _REWARD_SCALE or _REWARD_OFFSET the device
actors and the evaluation episodes step that task in the fork's wrapper's place (task_create).
Under Config.DDPG_SOFT (with DDPG_TWIN) the actor's head is [300, 2A], a mean and a log standard deviation per action, every
prediction with the handle's own noise is tanh of a Gaussian sample drawn in the kernel, and the handle has one more variable,
actor_soft/log_alpha, the learned temperature (soft_create).
"""
import ctypes as C
import os
import threading

import numpy as np

from Config import Config, DEVICE_DDPG_TASK_DEFAULTS, _resolve_soft
from NetworkVP import _device_ordinal
from NetworkVP_vecnet import DeviceActors, NativeHandle
import _native as nat

H1, H2 = 400, 300
ACTOR_TRAINABLE = ("actor_fc1/W", "actor_fc1/b", "actor_norm1/beta", "actor_norm1/gamma", "actor_fc2/W", "actor_fc2/b",
                   "actor_norm2/beta", "actor_norm2/gamma", "actor_output/W", "actor_output/b")
CRITIC_TRAINABLE = ("critic_fc1/W", "critic_fc1/b", "critic_norm1/beta", "critic_norm1/gamma", "critic_fc2/W", "critic_fc2/b",
                    "critic_norm2/W", "critic_norm2/b", "critic_output/W", "critic_output/b")
TRAINABLE = ACTOR_TRAINABLE + CRITIC_TRAINABLE
TWIN_TRAINABLE = tuple("critic2_" + k[len("critic_"):] for k in CRITIC_TRAINABLE)      # of a handle with twin critics
VALUE, TARGET, SLOT_A, SLOT_B, GRAD = range(5)


POPART_STATS = ("critic_popart/mu", "critic_popart/nu")      # of a handle with PopArt: not trainable, behind the 26
SOFT_LOG_ALPHA = "actor_soft/log_alpha"                      # of a handle with the soft actor-critic: trainable, behind the 38

# The task of the device actors: (bound, time_limit, reset_observation, reward_scale, reward_offset).  FORK_TASK is
# EnvironmentPend.Environment's, what a handle without a task steps.
TASK_BOUNDS = ('wrap', 'clip')
TASK_TIME_LIMITS = ('terminal', 'truncate')
FORK_TASK = tuple(default for _, default in DEVICE_DDPG_TASK_DEFAULTS)      # ('wrap', 'terminal', False, 0.005, -1.0)


def config_task():
    """Config's five DEVICE_DDPG task keys as a task tuple; a task is attached when it != FORK_TASK, which is Config's own test
    of a non-default key (_refuse_task_without_device_ddpg)."""
    return tuple(getattr(Config, key) for key, _ in DEVICE_DDPG_TASK_DEFAULTS)


def param_shapes(state_dim, num_actions, twin=False, atoms=None, popart=False, soft=False):
    S, A = int(state_dim), int(num_actions)
    if soft:                                # the Gaussian head and the temperature (on a twin handle)
        shapes = param_shapes(S, A, twin)
        shapes.update({"actor_output/W": (H2, 2 * A), "actor_output/b": (2 * A,), SOFT_LOG_ALPHA: (1,)})
        return shapes
    if popart:                              # + the two statistics (never with a twin or an atom head)
        shapes = param_shapes(S, A)
        shapes.update({k: (1,) for k in POPART_STATS})
        return shapes
    if atoms is not None:                   # a distributional critic: the head has one output per atom
        shapes = param_shapes(S, A, twin)
        shapes.update({"critic_output/W": (H2, int(atoms)), "critic_output/b": (int(atoms),)})
        return shapes
    if twin:                                # + critic 2's, shaped as the critic's
        shapes = param_shapes(S, A)
        shapes.update(zip(TWIN_TRAINABLE, [shapes[k] for k in CRITIC_TRAINABLE]))
        return shapes
    return {"actor_fc1/W": (S, H1), "actor_fc1/b": (H1,), "actor_norm1/beta": (H1,), "actor_norm1/gamma": (H1,),
            "actor_fc2/W": (H1, H2), "actor_fc2/b": (H2,), "actor_norm2/beta": (H2,), "actor_norm2/gamma": (H2,),
            "actor_output/W": (H2, A), "actor_output/b": (A,),
            "critic_fc1/W": (S, H1), "critic_fc1/b": (H1,), "critic_norm1/beta": (H1,), "critic_norm1/gamma": (H1,),
            "critic_fc2/W": (H1, H2), "critic_fc2/b": (H2,), "critic_norm2/W": (A, H2), "critic_norm2/b": (H2,),
            "critic_output/W": (H2, 1), "critic_output/b": (1,)}


def _truncated_normal(rng, shape, stddev):
    out = rng.normal(0.0, stddev, size=shape)
    bad = np.abs(out) > 2 * stddev
    while bad.any():                        # resample beyond two standard deviations
        out[bad] = rng.normal(0.0, stddev, size=int(bad.sum()))
        bad = np.abs(out) > 2 * stddev
    return out


def _draw(rng, name, shape):
    """tflearn's defaults as DESIGN.md 8f restates them (the one place): W truncated normal 0.02, the two output layers
    U(-0.003, 0.003) (NetworkDDPG.py:226,408), b = 0, beta = 0, gamma ~ N(1, 0.002)."""
    if name in ("actor_output/W", "critic_output/W", "critic2_output/W"):
        return rng.uniform(-0.003, 0.003, size=shape)
    if name.endswith("/W"):
        return _truncated_normal(rng, shape, 0.02)
    if name.endswith("/gamma"):
        return rng.normal(1.0, 0.002, size=shape)
    return np.zeros(shape)


def initial_arena(state_dim, num_actions, seed, tau=None, twin=False, atoms=None, soft=False):
    """-> (online, target): dicts of f32 arrays for the 20 trainable variables, drawn from one PCG64(seed) stream in variable
    order, the online networks first (actor, critic), then independently drawn targets in the same order.  The reference does
    not copy the online weights: it runs ONE soft update on those targets (NetworkDDPG.py:17-21), restated here.
    twin: critic 2's ten as well, drawn after all of those from the same stream (online, then targets), so that the 20 are
    what they are without it.  atoms: critic_output/W and /b at a distributional critic's shapes, drawn in their place of
    the stream.  soft: actor_output/W and /b at the Gaussian head's shapes, drawn by the rule of that variable in its place."""
    tau = Config.tau if tau is None else tau
    rng = np.random.Generator(np.random.PCG64(seed))
    shapes = param_shapes(state_dim, num_actions, twin, atoms, soft=soft)
    online, target = {}, {}
    for names in (TRAINABLE,) + ((TWIN_TRAINABLE,) if twin else ()):
        online.update({k: _draw(rng, k, shapes[k]).astype(np.float32) for k in names})
        target0 = {k: _draw(rng, k, shapes[k]).astype(np.float32) for k in names}
        target.update({k: (np.float32(tau) * online[k] + np.float32(1.0 - tau) * target0[k]).astype(np.float32) for k in names})
    return online, target


class Network(DeviceActors, NativeHandle):
    PREFIX = "ga3c_ddpg"
    soft = False                            # the handle has the soft actor-critic (set by __init__ from Config.DDPG_SOFT)

    def __init__(self, device, model_name, num_actions, state_dim, max_batch=None, predict_lanes=None, replay_capacity=None):
        self.device = device
        self.model_name = model_name
        self.num_actions = int(num_actions)
        self.state_dim = tuple(state_dim) if np.ndim(state_dim) else (int(state_dim),)
        if len(self.state_dim) != 1:
            raise ValueError("state_dim %r is not a vector" % (state_dim,))
        self.S = int(self.state_dim[0])
        self.learning_rate = Config.LEARNING_RATE_START
        self.beta = Config.BETA_START
        if Config.add_uncertainity:
            raise ValueError("add_uncertainity is not supported")
        if Config.DDPG_CRITIC_LOSS not in ('fork', 'paired'):
            raise ValueError("DDPG_CRITIC_LOSS=%r: 'fork' or 'paired'" % (Config.DDPG_CRITIC_LOSS,))
        if max_batch is None:
            max_batch = max(Config.PREDICTION_BATCH_SIZE, Config.TRAINING_MIN_BATCH_SIZE, Config.TIME_MAX + 1)
        self.max_batch = int(max_batch)
        self._lib = nat.hip_lib()
        cfg = nat.DdpgConfig()
        cfg.device = _device_ordinal(device)
        cfg.state_dim = self.S
        cfg.num_actions = self.num_actions
        cfg.max_batch = self.max_batch
        cfg.replay_capacity = int(replay_capacity or Config.REPLAY_BUFFER_SIZE)
        cfg.predict_lanes = int(predict_lanes or 2 * max(Config.PREDICTORS, 4 if Config.DYNAMIC_SETTINGS else 1) + 2)
        cfg.flags = ((nat.DDPG_FUTURE_REWARD if Config.DDPG_FUTURE_REWARD_CALC else 0)
                     | (nat.DDPG_LOSS_PAIRED if Config.DDPG_CRITIC_LOSS == 'paired' else 0)
                     | (nat.DDPG_GRAD_CLIP if Config.USE_GRAD_CLIP else 0)
                     | (0 if Config.RMSPROP else nat.DDPG_CRITIC_ADAM)
                     | (nat.DDPG_OU_NOISE if Config.add_OUnoise and not Config.DDPG_SOFT else 0))
        cfg.tau, cfg.gamma = Config.tau, Config.gamma
        cfg.actor_lr, cfg.critic_lr = Config.actor_lr, Config.critic_lr
        cfg.rmsprop_decay = Config.RMSPROP_DECAY
        cfg.rmsprop_momentum = Config.RMSPROP_MOMENTUM
        cfg.rmsprop_epsilon = Config.RMSPROP_EPSILON
        cfg.grad_clip_norm = Config.GRAD_CLIP_NORM
        cfg.ou_sigma, cfg.ou_theta, cfg.ou_dt = Config.OU_SIGMA, Config.OU_THETA, Config.OU_DT
        cfg.seed = Config.RANDOM_SEED
        handle = C.c_void_p()
        nat.check(self._fn("create")(C.byref(cfg), C.byref(handle)), "ga3c_ddpg_create")
        self._h = handle
        self.replay_capacity = cfg.replay_capacity
        self.twin = bool(Config.DDPG_TWIN)
        if self.twin:                           # before the initial values: it adds critic 2's variables
            self._call("twin_create", int(Config.DDPG_POLICY_DELAY), float(Config.DDPG_TARGET_NOISE),
                       float(Config.DDPG_TARGET_NOISE_CLIP), int(Config.RANDOM_SEED))
        self.soft = bool(Config.DDPG_SOFT)
        if self.soft:                           # after the twin, before the initial values: it widens the actor's head
            _resolve_soft(self.num_actions)
            ent = Config.DDPG_SOFT_TARGET_ENTROPY
            self._call("soft_create", float(np.log(Config.DDPG_SOFT_ALPHA)), float(Config.DDPG_SOFT_ALPHA_LR),
                       float(-self.num_actions if ent is None else ent), float(Config.DDPG_SOFT_LOG_STD_MIN),
                       float(Config.DDPG_SOFT_LOG_STD_MAX), int(Config.RANDOM_SEED + 3))
        self.dist = bool(Config.DDPG_DISTRIBUTIONAL)
        if self.dist:                           # before the initial values: it reshapes the critic's head
            self._call("dist_create", int(Config.DDPG_ATOMS), float(Config.DDPG_V_MIN), float(Config.DDPG_V_MAX))
        online, target = initial_arena(self.S, self.num_actions, Config.RANDOM_SEED, twin=self.twin,
                                       atoms=int(Config.DDPG_ATOMS) if self.dist else None, soft=self.soft)
        for k in TRAINABLE + (TWIN_TRAINABLE if self.twin else ()):
            self.set_variable_value(k, online[k], VALUE)
            self.set_variable_value(k, target[k], TARGET)
        self._log_lock = threading.Lock()
        self.logging = (0.0, 0.0)               # Q_max, Q_avg of the last step (NetworkDDPG.py:98)
        self.popart = bool(Config.DDPG_POPART)
        if self.popart:                         # after the initial values: it adds the two statistics, 0 and 1, and moves no weight
            self._call("popart_create", float(Config.DDPG_POPART_BETA), float(Config.DDPG_POPART_SIGMA_MIN),
                       float(Config.DDPG_POPART_SIGMA_MAX))
        self.prioritized = bool(Config.PRIORITIZED_REPLAY)
        self.replay_beta = Config.PRIORITIZED_REPLAY_BETA_START      # exponent of the importance weights; Server.main anneals it
        if self.prioritized:
            self._call("priorities_create", float(Config.PRIORITIZED_REPLAY_ALPHA), float(Config.PRIORITIZED_REPLAY_EPS),
                       int(Config.REPLAY_BUFFER_RANDOM_SEED))
        self.nstep = int(Config.DDPG_NSTEP)
        if self.nstep > 1:                      # before actors_create, which sizes the environments' windows
            self._call("nstep_create", self.nstep)
        self.task = None                        # None: the fork's task, and nothing is asked of the library
        if config_task() != FORK_TASK:          # before actors_create and eval_create, which choose their kernels
            self.task_create(*config_task())

    # ---- variables: which = VALUE, TARGET, SLOT_A, SLOT_B (RMSProp ms / mom or Adam m / v), GRAD -----------------------
    def set_global_step(self, step):
        self._call("set_step", int(step))

    def get_target_names(self):
        n = self._fn("num_params")(self._h)
        return [self._fn("target_name")(self._h, i).decode() + ":0" for i in range(n)]

    def _param_info(self, name):
        count, ndim, trainable = C.c_int64(), C.c_int32(), C.c_int32()
        shape = (C.c_int64 * 4)()
        self._call("param_info", name.encode(), C.byref(count), C.byref(ndim), shape, C.byref(trainable))
        return count.value, tuple(shape[d] for d in range(ndim.value)), bool(trainable.value)

    def get_variable_value(self, name, which=VALUE):
        count, shape, _ = self._param_info(name)
        out = np.empty(count, dtype=np.float32)
        self._call("get_param", name.encode(), which, nat.ptr(out), count)
        return out.reshape(shape)

    def set_variable_value(self, name, value, which=VALUE):
        flat = nat.as_f32(value).ravel()
        self._call("set_param", name.encode(), which, nat.ptr(flat), flat.size)

    # ---- noise -----------------------------------------------------------------------------------
    def _noise_args(self, noise):
        """noise: None = the handle's own process (one step per call), False = none, or a vector [A]."""
        if noise is None:
            return nat.DDPG_NOISE_OWN, None, None
        if noise is False:
            return nat.DDPG_NOISE_NONE, None, None
        v = nat.as_f32(noise).ravel()
        if v.size != self.num_actions:
            raise ValueError("noise of %d elements for %d actions" % (v.size, self.num_actions))
        return nat.DDPG_NOISE_GIVEN, nat.ptr(v), v

    def noise_step(self):
        """One step of the handle's OU process -> (x[A], n[A]): the new state and the normal draws it used."""
        x, n = np.empty(self.num_actions, np.float32), np.empty(self.num_actions, np.float32)
        self._call("noise_step", nat.ptr(x), nat.ptr(n))
        return x, n

    # ---- inference ---------------------------------------------------------------------------
    def predict(self, x, noise=None):
        x, b = self._rows(x)
        mode, nptr, _keep = self._noise_args(noise)
        a = np.empty((b, self.num_actions), np.float32)
        self._call("predict", nat.ptr(x), b, mode, nptr, nat.ptr(a))
        return a

    def predict_p_and_v(self, x):
        """(action, action), as the reference returns it (NetworkDDPG.py:106-111)."""
        a = self.predict(x)
        return [a, a]

    def predict_single(self, x):
        return self.predict(x[None, :])[0]

    # ---- zero-copy intake from the shared-memory transport -------------------------------------------
    def predict_offsets(self, offsets):
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        b = offsets.size
        p = np.empty((b, self.num_actions), np.float32)
        v = np.empty(b, np.float32)
        self._call("predict_gather", nat.ptr(offsets, nat.i64p), b, 0, nat.ptr(p), nat.ptr(v), None)
        return [p, p]

    # ---- replay memory (replay_buffer.py:16-55, a ring in HBM) ------------------------------------------
    def replay_add(self, s, a, r, done, s2):
        """Appends the rows -> (rows held, rows ever added)."""
        s, n = self._rows(s)
        s2, _ = self._rows(s2)
        a = nat.as_f32(a).reshape(n, self.num_actions)
        r, done = nat.as_f32(r).ravel(), nat.as_f32(done).ravel()
        size, total = C.c_int64(), C.c_int64()
        self._call("replay_add", nat.ptr(s), nat.ptr(a), nat.ptr(r), nat.ptr(done), nat.ptr(s2), n,
                   C.byref(size), C.byref(total))
        return size.value, total.value

    def replay_add_offsets(self, offsets, r, a):
        """Rows `s | s2 | done` of the registered transport by byte offset -> (rows held, rows ever added)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = offsets.size
        r, a = nat.as_f32(r).ravel(), nat.as_f32(a).reshape(n, self.num_actions)
        size, total = C.c_int64(), C.c_int64()
        self._call("replay_add_gather", nat.ptr(offsets, nat.i64p), nat.ptr(r), nat.ptr(a), n, C.byref(size), C.byref(total))
        return size.value, total.value

    def replay_get(self, slot):
        s, s2 = np.empty(self.S, np.float32), np.empty(self.S, np.float32)
        a = np.empty(self.num_actions, np.float32)
        r, done = C.c_float(), C.c_float()
        self._call("replay_get", int(slot), nat.ptr(s), nat.ptr(a), C.byref(r), C.byref(done), nat.ptr(s2))
        return s, a, np.float32(r.value), np.float32(done.value), s2

    def replay_size(self):
        size, total = C.c_int64(), C.c_int64()
        self._call("replay_size", C.byref(size), C.byref(total))
        return size.value, total.value

    # ---- training ----------------------------------------------------------------------------
    def _five(self, x, y_r, a, x2, done):
        s, b = self._rows(x)
        s2, _ = self._rows(x2)
        return (s, nat.as_f32(a).reshape(b, self.num_actions), nat.as_f32(y_r).ravel(), nat.as_f32(done).ravel(), s2, b)

    def train(self, x, y_r, a, x2, done, trainer_id=0, noise=None):
        """train_DDPG(s = x, a, r = y_r, done, s2 = x2) (NetworkDDPG.py:61-62)."""
        s, a, r, d, s2, b = self._five(x, y_r, a, x2, done)
        mode, nptr, _keep = self._noise_args(noise)
        q = np.empty(2, np.float32)
        self._call("train", nat.ptr(s), nat.ptr(a), nat.ptr(r), nat.ptr(d), nat.ptr(s2), b,
                   float(self.learning_rate), mode, nptr, nat.ptr(q))
        self.logging = (float(q[0]), float(q[1]))
        return self.logging

    def train_replay(self, slots, stamp=-1, noise=None):
        """One step on ring slots; stamp: the ring's `total` when they were sampled (a slot written since raises StateLost)."""
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        mode, nptr, _keep = self._noise_args(noise)
        q = np.empty(2, np.float32)
        self._call("train_replay", nat.ptr(slots, nat.i32p), slots.size, int(stamp),
                   float(self.learning_rate), mode, nptr, nat.ptr(q))
        self.logging = (float(q[0]), float(q[1]))
        return self.logging

    # ---- prioritised replay (Config.PRIORITIZED_REPLAY) ---------------------------------------
    def train_prioritized(self, batch, noise=None):
        """One step on `batch` rows the handle draws by priority, weighted by (N P(i)) ^ -replay_beta -> (Q_max, Q_avg).
        The slots it drew are in last_slots afterwards."""
        mode, nptr, _keep = self._noise_args(noise)
        q, slots = np.empty(2, np.float32), np.empty(int(batch), np.int32)
        self._call("train_prioritized", int(batch), float(self.replay_beta), float(self.learning_rate), mode, nptr,
                   nat.ptr(q), nat.ptr(slots, nat.i32p))
        self.last_slots = slots
        self.logging = (float(q[0]), float(q[1]))
        return self.logging

    def sample_prioritized(self, batch):
        """One draw and nothing else -> (slots int32 [batch], weights f32 [batch])."""
        slots, w = np.empty(int(batch), np.int32), np.empty(int(batch), np.float32)
        self._call("sample_prioritized", int(batch), float(self.replay_beta), nat.ptr(slots, nat.i32p), nat.ptr(w))
        return slots, w

    def priorities(self):
        """-> (pa f32 [replay_capacity]: priority ^ alpha by ring slot, max_pa)."""
        pa, top = np.empty(self.replay_capacity, np.float32), C.c_float()
        self._call("priorities_get", nat.ptr(pa), C.byref(top))
        return pa, np.float32(top.value)

    def set_priorities(self, pa, max_pa):
        pa = nat.as_f32(pa).ravel()
        if pa.size != self.replay_capacity:
            raise ValueError("%d priorities for %d ring slots" % (pa.size, self.replay_capacity))
        self._call("priorities_set", nat.ptr(pa), float(max_pa))

    def time_prioritized(self, batch, iters):
        """Milliseconds of `iters` resident prioritised steps of `batch` rows."""
        ms = C.c_float()
        self._call("time_prioritized", int(batch), int(iters), float(self.replay_beta), float(self.learning_rate), C.byref(ms))
        return ms.value

    # ---- distributional critic (Config.DDPG_DISTRIBUTIONAL) ---------------------------------
    def dist_info(self):
        """-> (atoms, v_min, v_max) of the handle's critic; atoms = 1 without a distributional one."""
        n, lo, hi = C.c_int32(), C.c_float(), C.c_float()
        self._call("dist_info", C.byref(n), C.byref(lo), C.byref(hi))
        return n.value, lo.value, hi.value

    # ---- soft actor-critic (Config.DDPG_SOFT) -------------------------------------------------
    def soft_info(self):
        """-> (log_alpha, target_entropy, mean_logp, predictions): the temperature's logarithm as it stands, the entropy it is
        steered to, the mean log-density of the last policy step's samples, and the count of predictions that drew their own noise."""
        la, ent, lp, n = C.c_float(), C.c_float(), C.c_float(), C.c_int64()
        self._call("soft_info", C.byref(la), C.byref(ent), C.byref(lp), C.byref(n))
        return la.value, ent.value, lp.value, n.value

    def log_soft(self, training_step):
        """training_step, alpha, mean_logp appended to logs/<model>/soft.csv, beside eval.csv."""
        la, _, lp, _ = self.soft_info()
        os.makedirs("logs/%s" % self.model_name, exist_ok=True)
        with self._log_lock:
            with open("logs/%s/soft.csv" % self.model_name, "a") as f:
                f.write("%d,%.9g,%.9g\n" % (training_step, float(np.exp(la)), lp))

    # ---- PopArt (Config.DDPG_POPART) ----------------------------------------------------------
    def popart_info(self):
        """-> (beta, mu, nu, sigma): the step of the statistics, the targets' running first and second moment, and the scale
        they give.  The critic's output n stands for the return sigma n + mu."""
        beta, mu, nu, sigma = C.c_float(), C.c_float(), C.c_float(), C.c_float()
        self._call("popart_info", C.byref(beta), C.byref(mu), C.byref(nu), C.byref(sigma))
        return beta.value, mu.value, nu.value, sigma.value

    def log_popart(self, training_step):
        """training_step, mu, nu, sigma appended to logs/<model>/popart.csv, beside eval.csv."""
        _, mu, nu, sigma = self.popart_info()
        os.makedirs("logs/%s" % self.model_name, exist_ok=True)
        with self._log_lock:
            with open("logs/%s/popart.csv" % self.model_name, "a") as f:
                f.write("%d,%.9g,%.9g,%.9g\n" % (training_step, mu, nu, sigma))

    # ---- n-step returns (Config.DDPG_NSTEP) ------------------------------------------------
    def nstep_create(self, n):
        """Attaches n-step state to a handle that has none (Config.DDPG_NSTEP = 1) and no device actors yet."""
        self._call("nstep_create", int(n))
        self.nstep = int(n)

    def nstep_discounts(self):
        """-> f32 [replay_capacity]: the discount of the row in each ring slot, gamma^m."""
        disc = np.empty(self.replay_capacity, np.float32)
        self._call("nstep_get", nat.ptr(disc), disc.size)
        return disc

    def set_nstep_discounts(self, disc):
        disc = nat.as_f32(disc).ravel()
        if disc.size != self.replay_capacity:
            raise ValueError("%d discounts for %d ring slots" % (disc.size, self.replay_capacity))
        self._call("nstep_set", nat.ptr(disc), disc.size)

    # ---- the task (Config.DEVICE_DDPG_ACTION_BOUND .. _REWARD_OFFSET) ----------------------------------
    def task_create(self, bound, time_limit, reset_observation, reward_scale, reward_offset):
        """Attaches a task to a handle that has none and neither device actors nor evaluation episodes yet."""
        if bound not in TASK_BOUNDS:
            raise ValueError("bound=%r: 'wrap' or 'clip'" % (bound,))
        if time_limit not in TASK_TIME_LIMITS:
            raise ValueError("time_limit=%r: 'terminal' or 'truncate'" % (time_limit,))
        self._call("task_create", TASK_BOUNDS.index(bound), TASK_TIME_LIMITS.index(time_limit), int(bool(reset_observation)),
                   float(reward_scale), float(reward_offset))
        self.task = self.task_info()

    def task_info(self):
        """-> (bound, time_limit, reset_observation, reward_scale, reward_offset) as the handle holds them."""
        bound, limit, reset = C.c_int32(), C.c_int32(), C.c_int32()
        scale, offset = C.c_double(), C.c_double()
        self._call("task_info", C.byref(bound), C.byref(limit), C.byref(reset), C.byref(scale), C.byref(offset))
        return TASK_BOUNDS[bound.value], TASK_TIME_LIMITS[limit.value], bool(reset.value), scale.value, offset.value

    def task_destroy(self):
        self._call("task_destroy")
        self.task = None

    # ---- device actors (Config.DEVICE_DDPG) ------------------------------------------------
    # what ga3c_ddpg_actors_get names (NetworkVP_vecnet.DeviceActors); "slots" has one row per row of a train step
    ACTOR_FIELDS = {"phys": (np.float64, 2), "elapsed": (np.int32, 1), "draws": (np.uint64, 1), "obs": (np.float32, 3),
                    "action": (np.float32, "A"), "reward": (np.float64, 1), "done": (np.int32, 1), "slots": (np.int32, 1)}
    ACTOR_SCALARS = {"batch": np.int32, "draw_seed": np.int64, "nstep": np.int32, "nstep_count": np.int64}
    ACTOR_ROWS = {"slots": "batch"}

    # ... and, on a handle whose actors have per-environment noise (Config.DEVICE_DDPG_NOISE = 'per_env'), these
    # too; the handle's own ACTOR_FIELDS / ACTOR_SCALARS list them while it has it: without it the library knows no such names
    NOISE_FIELDS = {"noise_x": (np.float32, "A"), "noise_n": (np.float32, "A")}
    NOISE_SCALARS = {"noise_count": np.int64}
    # ... and on a handle with the soft actor-critic the actors' last draws
    SOFT_FIELDS = {"soft_eps": (np.float32, "A")}

    def actors_create(self, n, time_max=None, discount=None, seed=None, updates=None, batch=None, draw_seed=None, noise=None,
                      noise_seed=None, noise_reset=None):
        """n Pendulum-v0 environments on the handle, with Config's train-step rows, updates per actor step, draw seed and
        exploration noise ('shared' or 'per_env', its seed RANDOM_SEED + 2: + 1 is the evaluation's) unless given.  time_max and
        discount are ThreadDeviceAgents' call shape: a ring of transitions has neither."""
        noise = Config.DEVICE_DDPG_NOISE if noise is None else noise
        if noise not in ('shared', 'per_env'):
            raise ValueError("noise=%r: 'shared' or 'per_env'" % (noise,))
        self._call("actors_create", int(n), int(Config.DEVICE_DDPG_UPDATES if updates is None else updates),
                   int(Config.RANDOM_SEED if seed is None else seed))
        self.num_actors = int(n)
        self.actors_set("batch", min(self.max_batch, int(Config.TRAINING_MIN_BATCH_SIZE if batch is None else batch)))
        self.actors_set("draw_seed", Config.REPLAY_BUFFER_RANDOM_SEED if draw_seed is None else draw_seed)
        if self.soft:
            self.ACTOR_FIELDS = dict(type(self).ACTOR_FIELDS, **self.SOFT_FIELDS)
        if noise == 'per_env':
            self.envnoise_create(noise_seed, noise_reset)

    def envnoise_create(self, seed=None, reset=None):
        """Gives every environment of the handle's device actors a noise process of its own."""
        self._call("envnoise_create", int(Config.RANDOM_SEED + 2 if seed is None else seed),
                   int(bool(Config.DEVICE_DDPG_NOISE_RESET if reset is None else reset)))
        self.ACTOR_FIELDS = dict(type(self).ACTOR_FIELDS, **self.NOISE_FIELDS)
        self.ACTOR_SCALARS = dict(type(self).ACTOR_SCALARS, **self.NOISE_SCALARS)

    def envnoise_destroy(self):
        self._call("envnoise_destroy")
        self._forget_envnoise()

    def _forget_envnoise(self):
        self.__dict__.pop("ACTOR_FIELDS", None)
        self.__dict__.pop("ACTOR_SCALARS", None)

    def actors_destroy(self):
        super().actors_destroy()
        self._forget_envnoise()

    def actors_run(self, steps, train=True, noise=None):
        """`steps` actor steps, each followed by DEVICE_DDPG_UPDATES train steps once the ring holds more than a batch, at the
        model's learning_rate and replay_beta -> (agent steps, train steps, rows trained, episodes finished)."""
        mode, nptr, _keep = self._noise_args(noise)
        stats, q = np.zeros(4, np.int64), np.empty(2, np.float32)
        self._call("actors_run", int(steps), float(self.learning_rate), float(self.replay_beta), int(bool(train)), mode, nptr,
                   nat.ptr(stats, nat.i64p), nat.ptr(q))
        if stats[1]:
            self.logging = (float(q[0]), float(q[1]))
        return tuple(int(t) for t in stats)

    # ---- evaluation episodes (Config.DEVICE_DDPG_EVAL_ENVS) ---------------------------------
    # what ga3c_ddpg_eval_get names: (dtype, shape of an environment's row); the trace_* ones need trace=True at eval_create
    EVAL_STEPS = 200
    EVAL_FIELDS = {"start": (np.float64, (2,)), "phys": (np.float64, (2,)), "trace_phys": (np.float64, (200, 2)),
                   "trace_obs": (np.float32, (200, 3)), "trace_action": (np.float32, (200,)),
                   "trace_reward": (np.float64, (200,))}

    def eval_create(self, n=None, seed=None, trace=False):
        """n Pendulum-v0 environments for noise-free episodes, whose start states are drawn once from `seed`."""
        n = int(Config.DEVICE_DDPG_EVAL_ENVS if n is None else n)
        self._call("eval_create", n, int(Config.RANDOM_SEED + 1 if seed is None else seed), int(bool(trace)))
        self.num_eval = n

    def eval_destroy(self):
        self._call("eval_destroy")

    def eval_run(self, steps=200, target=False):
        """One episode of `steps` steps per environment under the online actor (target: its target copy), from the start
        states -> f64 [n]: the sum of each environment's rewards."""
        totals = np.empty(self.num_eval, np.float64)
        self._call("eval_run", int(steps), int(bool(target)), nat.ptr(totals, nat.f64p))
        return totals

    def eval_get(self, name):
        if name == "elapsed_ms":                    # of the last run's kernel, between two events on the handle's stream
            out = np.zeros(1, np.float32)
            self._call("eval_get", name.encode(), out.ctypes.data_as(C.c_void_p), out.nbytes)
            return float(out[0])
        dtype, shape = self.EVAL_FIELDS[name]
        out = np.zeros((self.num_eval,) + shape, dtype)
        self._call("eval_get", name.encode(), out.ctypes.data_as(C.c_void_p), out.nbytes)
        return out

    def eval_set(self, name, value):
        value = np.ascontiguousarray(value, dtype=self.EVAL_FIELDS[name][0])
        self._call("eval_set", name.encode(), value.ctypes.data_as(C.c_void_p), value.nbytes)

    def log_eval(self, training_step, totals, steps):
        """training_step, n, steps, mean, min, max, mean_gym_return appended to logs/<model>/eval.csv.  The last undoes the
        reward's scale and offset per step (the wrapper's r * 0.005 - 1 without a task): the return gym's Pendulum-v0 would
        report for the same episode."""
        totals = np.asarray(totals, np.float64)
        mean = float(totals.mean())
        scale, offset = (getattr(self, "task", None) or FORK_TASK)[3:]
        os.makedirs("logs/%s" % self.model_name, exist_ok=True)
        with self._log_lock:
            with open("logs/%s/eval.csv" % self.model_name, "a") as f:
                f.write("%d,%d,%d,%.17g,%.17g,%.17g,%.17g\n" % (training_step, totals.size, steps, mean, float(totals.min()),
                                                               float(totals.max()), (mean - steps * offset) / scale))

    def compute(self, x, y_r, a, x2, done, stop_after, noise=None):
        s, a, r, d, s2, b = self._five(x, y_r, a, x2, done)
        mode, nptr, _keep = self._noise_args(noise)
        q = np.empty(2, np.float32)
        self._call("compute", nat.ptr(s), nat.ptr(a), nat.ptr(r), nat.ptr(d), nat.ptr(s2), b,
                   float(self.learning_rate), mode, nptr, int(stop_after), nat.ptr(q))
        return float(q[0]), float(q[1])

    def time_resident(self, mode, batch, iters):
        """Milliseconds of `iters` resident calls (mode 0 predict, 1 train_replay) on ring slots 0 .. batch-1."""
        ms = C.c_float()
        self._call("time_resident", int(mode), int(batch), int(iters), float(self.learning_rate), C.byref(ms))
        return ms.value

    # ---- logging / checkpoints -----------------------------------------------------------------
    def log(self, x=None, y_r=None, a=None, training_step=0, feed_dict=None, offsets=None, frames=None):
        """LearningRate, Q_max, Q_avg (NetworkDDPG.py:122,133-134) appended to logs/<model>/scalars.csv."""
        q_max, q_avg = self.logging
        os.makedirs("logs/%s" % self.model_name, exist_ok=True)
        with self._log_lock:
            with open("logs/%s/scalars.csv" % self.model_name, "a") as f:
                f.write("%d,%.8g,%.8g,%.8g\n" % (training_step, self.learning_rate, q_max, q_avg))
        if self.popart:                         # scalars.csv keeps its four columns; Q above is in return units
            self.log_popart(training_step)
        if self.soft:
            self.log_soft(training_step)
