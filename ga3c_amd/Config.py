"""Global settings of the GA3C engine, read as class attributes exactly like the reference's
Config (/root/reference/ga3c/Config.py:27-202) and overridable from argv as KEY=VALUE
(GA3C.py:39-43).  Names and meanings are the reference's; defaults are the ones SURVEY.md §8-d
fixes for the 84x84x4 Atari path (the fork's own defaults target Pendulum), and the block at the
end adds the knobs this engine needs (devices, transport, return mode).
"""
import math
import os


class Config:
    # ---- what to run -------------------------------------------------------------------------
    GAME = 'PongDeterministic-v4'       # gym id, used by FRAME_SOURCE = 'gym' only; the offline sources are synthetic.
                                        # 'Pendulum-v0' (the fork's own default): the vector-state network and the
                                        # restated Pendulum (NetworkVP_vector.py, EnvironmentPend.py).
                                        # 'CartPole-v0': the softmax head on a vector state and the restated CartPole
                                        # (NetworkVP_discrate.py, EnvironmentCart.py)
    PLAY_MODE = False                   # greedy actions, no training, one agent (GA3C.py:46-54)
    TRAIN_MODELS = True
    LOAD_CHECKPOINT = False
    LOAD_EPISODE = 0                    # 0 = latest checkpoint

    # ---- workers (initial values when DYNAMIC_SETTINGS is on) ---------------------------------
    AGENTS = 32
    HUMAN_REF_AGENTS = 0                # pyperrace-only in the reference; kept for argv compatibility
    PREDICTORS = 2
    TRAINERS = 2
    DEVICE = 'gpu:0'
    DYNAMIC_SETTINGS = False            # ThreadDynamicAdjustment random walk over NT/NP/NA
    DYNAMIC_SETTINGS_STEP_WAIT = 20
    DYNAMIC_SETTINGS_INITIAL_WAIT = 10

    # ---- algorithm ----------------------------------------------------------------------------
    DISCOUNTING = True
    DISCOUNT = 0.99
    TIME_MAX = 5                        # rollout cut (upstream Atari value, Config.py:77 comment)
    REWARD_CLIPPING = True
    USE_INTERMEDIATE_REWARD = False
    REWARD_MIN = -1
    REWARD_MAX = 1
    MAX_QUEUE_SIZE = 100
    PREDICTION_BATCH_SIZE = 128
    STACKED_FRAMES = 4
    IMAGE_WIDTH = 84
    IMAGE_HEIGHT = 84
    EPISODES = 400000
    ANNEALING_EPISODE_COUNT = 400000
    BETA_START = 0.01
    BETA_END = 0.01
    LEARNING_RATE_START = 0.0003
    LEARNING_RATE_END = 0.0003
    RMSPROP_DECAY = 0.99
    RMSPROP_MOMENTUM = 0.0
    RMSPROP_EPSILON = 0.1
    DUAL_RMSPROP = False                # one RMSProp optimizer per cost, cost_p and cost_v (NetworkVP_discrate.py:87-99); DESIGN §8
    USE_GRAD_CLIP = False
    GRAD_CLIP_NORM = 40.0
    LOG_EPSILON = 1e-6
    TRAINING_MIN_BATCH_SIZE = 0
    MIN_POLICY = 0.0
    USE_LOG_SOFTMAX = False
    DISCRATE_INPUT = True               # (sic) discrete action space: softmax policy head; derived, = not CONTINUOUS_INPUT
    CONTINUOUS_INPUT = False            # angle-output policy head, the action IS the prediction vector in (-1, 1]^A
                                        # (NetworkVP.py:92,95-105,175-204, ProcessAgent.py:134-137); DESIGN §8d
    USE_DDPG = False                    # NetworkDDPG.py with ThreadReplay.py (needs CONTINUOUS_INPUT); resolve_ddpg() applies what
    USE_REPLAY_MEMORY = False           # it implies (the reference's Config.py:160-178): USE_REPLAY_MEMORY, DISCOUNTING = False
    add_OUnoise = True                  # (sic) Ornstein-Uhlenbeck noise on every prediction of NetworkDDPG, which alone reads it
                                        # (the reference sets it True under USE_DDPG); switch off with `add_OUnoise=`.  Not read
                                        # under DDPG_SOFT: the stochastic policy's own sample is the exploration
    add_uncertainity = False            # (sic) an integer added to the prediction: not supported, raises
    REPLAY_BUFFER_SIZE = 1000000
    REPLAY_BUFFER_RANDOM_SEED = 12345
    REPLAY_MIN_QUEUE_SIZE = 2
    PRIORITIZED_REPLAY = False          # USE_DDPG only: the device draws a train step's rows in proportion to their TD error
                                        # (Schaul et al. 2016) instead of the replay thread drawing them uniformly; needs
                                        # DDPG_CRITIC_LOSS = 'paired' and REPLAY_BUFFER_SIZE <= 1048576
    PRIORITIZED_REPLAY_ALPHA = 0.6      # priority = (|y - q| + eps) ^ alpha: 0 draws uniformly, 1 in proportion to the error
    PRIORITIZED_REPLAY_BETA_START = 0.4     # exponent of the importance weights (N P(i)) ^ -beta on the critic's loss, annealed
    PRIORITIZED_REPLAY_BETA_END = 1.0       # over ANNEALING_EPISODE_COUNT episodes as LEARNING_RATE is; 1 undoes the bias
    PRIORITIZED_REPLAY_EPS = 0.01       # keeps a row with no error drawable
    DDPG_FUTURE_REWARD_CALC = True      # y = r + gamma q' on rows that are not done; False: y = r
    DDPG_CRITIC_LOSS = 'fork'           # 'fork': mean_square(y[B], q[B,1]) broadcasts, the critic regresses on mean(y), as the
                                        # reference computes it; 'paired': (q_i - y_i)^2
    DDPG_TWIN = False                   # USE_DDPG only: two critics, y from the smaller target value at a smoothed target action,
                                        # the actor and the targets stepped every DDPG_POLICY_DELAY-th train step (Fujimoto et
                                        # al. 2018, "TD3"); needs DDPG_CRITIC_LOSS = 'paired' 
    DDPG_POLICY_DELAY = 2               # a policy step every this many train steps (1..16)
    DDPG_TARGET_NOISE = 0.2             # sigma of the target smoothing: a~ = clip(actor_target(s2) + clip(sigma n, -c, c), -1, 1)
    DDPG_TARGET_NOISE_CLIP = 0.5        # ... and its c
    DDPG_SOFT = False                   # DDPG_TWIN only: soft actor-critic (Haarnoja et al. 2018).  The actor's head gives a mean and a
                                        # log standard deviation per action, the action is tanh of a Gaussian sample drawn in the
                                        # kernels, alpha x the entropy enters the critics' target and the actor's loss, and alpha is
                                        # learned towards DDPG_SOFT_TARGET_ENTROPY; num_actions <= 16
    DDPG_SOFT_ALPHA = 0.2               # the temperature's first value (finite, > 0)
    DDPG_SOFT_ALPHA_LR = 1.0            # factor on the annealed learning rate for log alpha's Adam, as actor_lr is (>= 0; 0 fixes alpha)
    DDPG_SOFT_TARGET_ENTROPY = None     # None: -num_actions
    DDPG_SOFT_LOG_STD_MIN = -20.0       # the head's log standard deviation is clamped into [DDPG_SOFT_LOG_STD_MIN, _MAX]
    DDPG_SOFT_LOG_STD_MAX = 2.0
    DDPG_NSTEP = 1                      # DEVICE_DDPG only: the ring's rows carry n-step returns, R = sum_{k<m} gamma^k r_k cut at an
                                        # episode's end, and y = R + gamma^m q'(s_m) (1..16; 1: one-step rows, as without it)
    DDPG_DISTRIBUTIONAL = False         # USE_DDPG only: the critic predicts a categorical distribution over DDPG_ATOMS fixed returns,
                                        # trained by cross-entropy against the projected target distribution; the actor ascends its
                                        # expectation (Barth-Maron et al. 2018, "D4PG"); needs DDPG_CRITIC_LOSS = 'paired', excludes
                                        # DDPG_TWIN
    DDPG_ATOMS = 51                     # atoms of the support (2..64)
    DDPG_V_MIN = -100.0                 # the support's ends.  EnvironmentPend hands on r 0.005 - 1 in [-1.09, -1]: the gamma = 0.99
    DDPG_V_MAX = 0.0                    # return over 200 steps lies above -94 and below 0
    DDPG_POPART = False                 # USE_DDPG only: the critic regresses on targets normalised by running statistics of the
                                        # targets, and its output layer is rescaled whenever they move so that no prediction does
                                        # (van Hasselt et al. 2016, "PopArt"); needs DDPG_CRITIC_LOSS = 'paired', excludes DDPG_TWIN
                                        # and DDPG_DISTRIBUTIONAL
    DDPG_POPART_BETA = 3e-4             # step of the statistics: mu' = (1 - beta) mu + beta mean(y), likewise for mean(y^2) (0..1)
    DDPG_POPART_SIGMA_MIN = 1e-4        # sigma = sqrt(nu - mu^2) is clamped into [DDPG_POPART_SIGMA_MIN, DDPG_POPART_SIGMA_MAX]
    DDPG_POPART_SIGMA_MAX = 1e6
    tau = 0.001
    gamma = 0.99
    actor_lr = 1.0                      # factors on the annealed learning rate; the later of the two assignments in the
    critic_lr = 10.0                    # reference's class body (Config.py:198-199)
    RMSPROP = True                      # critic optimizer: RMSProp (True) or Adam
    OU_SIGMA = 0.3                      # OrnsteinUhlenbeckActionNoise's defaults (NetworkDDPG.py:466)
    OU_THETA = 0.15
    OU_DT = 1e-2
    DENSE_LAYERS = (10, 10, 10, 10)     # widths of NetworkVP_discrate's dense layers (GAME = 'CartPole-v0'); `DENSE_LAYERS=64,64`
    DENSE_STACK = 'fork'                # 'fork': every layer reads the state and only the last reaches the heads, as the
                                        # reference builds them (NetworkVP_discrate.py:52-56); 'chained': layer i reads
                                        # layer i - 1
    USE_NETWORK_TESTER = False
    RANDOM_SEED = 12345

    # ---- logging / checkpoints ----------------------------------------------------------------
    TENSORBOARD = False                 # scalar log written as CSV under logs/<NETWORK_NAME>/
    TENSORBOARD_UPDATE_FREQUENCY = 1000
    SAVE_MODELS = True
    SAVE_FREQUENCY = 1000
    PRINT_STATS_FREQUENCY = 1
    STAT_ROLLING_MEAN_WINDOW = 1000
    RESULTS_FILENAME = 'results.txt'
    NETWORK_NAME = 'network'

    # ---- engine knobs (no counterpart in the reference) ----------------------------------------
    NUM_ACTIONS = 6                     # synthetic source only (Pong 6, Breakout 4, Boxing 18)
    MAX_SECONDS = 0                     # > 0: Server.main stops after this many seconds (the reference stops on EPISODES only)
    RETURN_MODE = 'fork'                # 'fork': ProcessAgent.py:69-84 bit-exact; 'nstep': upstream n-step
    STATE_TRANSPORT = 'u8'              # 'u8': ship uint8 frames, convert on GPU; 'f32': ship f32 states
    SYNTHETIC_EPISODE_LENGTH = 1000
    TRAIN_ROWS_MAX = 0                  # capacity of one train call; 0 = derive from the batch knobs
    HOGWILD = False                     # True: TRAINERS train lanes update the weights concurrently and unlocked,
                                        # as the reference's trainer threads do; False: synchronous steps (default)
    ZERO_COPY = True                    # GPU gathers states straight from the registered shm transport
    QUEUE_TIMEOUT_MS = 200              # workers re-check their exit flag this often
    NATIVE_PREDICTOR = True             # ThreadPredictor's loop in native code (ga3c_pq_serve) when ZERO_COPY is on
    PIPELINED_PREDICTOR = True          # ... answering batch k beside the GPU's work on batch k+1 (ga3c_pq_serve_pipelined)
    PIPELINED_FRAMES = False            # the same overlap for the frames loop (device frame queue): pays from ~500 agents per GPU on
    STATE_CACHE = True                  # the engine keeps the uint8 states its predictions read (a ring per agent in HBM) and
                                        # rollouts NAME their states (agent, request number) instead of carrying them: no second
                                        # trip over PCIe for training (needs ZERO_COPY, STATE_TRANSPORT = 'u8', the native
                                        # pipelined predictor and trainer loops; Server falls back without them)
    STATE_CACHE_DEPTH = 0               # states kept per agent (28,224 B each); 0 = four times an agent's fair share of the rows
                                        # in flight plus four rollouts, at least 64 (2.3 MB per agent at the defaults)
    STATE_CACHE_ACTIVE = False          # (set by Server for its agents: the cache is really in use)
    NATIVE_TRAINER = True               # ThreadTrainer's batch assembly in one native call (ga3c_tq_collect) when ZERO_COPY is on
    CPU_AFFINITY = 'auto'               # where server threads and agents run (Placement.py): 'auto' = as many CPUs as the cgroup's
                                        # quota allows, whole L3 domains next to the GPU; 'off'; or a list such as '0-15'
    AGENT_CPUS = None                   # (set by Server when the placement keeps CPUs apart for the agents)
    AGENT_SPIN_US = 0                   # > 0: an agent polls this long for its answer before it sleeps on the slot's futex
    PREDICTION_LINGER_US = 0            # > 0: a predictor holding fewer than PREDICTION_LINGER_BATCH requests after its
    PREDICTION_LINGER_BATCH = 0         # greedy drain keeps collecting this long (the reference never waits: 0)
    ROLLOUT_SLOTS = 0                   # rollout slots of the transport; 0 = MAX_QUEUE_SIZE (the reference's queue bound)
                                        # plus what the trainers keep while a zero-copy batch fills and trains
    FRAME_SOURCE = 'planes'             # 'gym': gym.make(GAME) frames (needs gym + ALE, absent offline: untested here);
                                        # 'planes': synthetic 84x84 uint8 planes; 'rgb': synthetic
                                        # emulator frames FRAME_HEIGHT x FRAME_WIDTH x 3 that go through the reference's
                                        # front-end (Environment.py:52-74: gray, bytescale, bilinear resize, frame queue)
    FRONTEND = 'host'                   # where that front-end runs for 'rgb' frames: 'host' = in the agent process
                                        # (ga3c_frame_preprocess), states shipped as before; 'device' = the agent ships
                                        # the raw frame, planes / frame queues / training rows stay in HBM.  With 'planes'
                                        # 'device' keeps only the 4-deep frame queue and the plane history in HBM: the agent
                                        # ships its newest 84x84 plane (7,056 B per step instead of a 28,224 B state, and
                                        # nothing at all for training)
    FRAME_HEIGHT = 210
    FRAME_WIDTH = 160
    FRAME_HISTORY = 0                   # planes of history per agent on the device; 0 = derived from the queue bounds
    DEVICE_AGENTS = 0                   # > 0 (GAME = 'CartPole-v0', or 'Pendulum-v0' with DEVICE_PENDULUM or DEVICE_DDPG): this many
                                        # environments, their rollouts and their training rows live in HBM and the server
                                        # steps them with HIP kernels; no agent process, predictor or trainer is started
                                        # (ThreadDeviceAgents.py)
    DEVICE_PENDULUM = False             # True: DEVICE_AGENTS steps Pendulum-v0.  An opt-in of its own because the regime differs:
                                        # the environments run in lockstep, one train step of N (TIME_MAX + 1) rows every
                                        # TIME_MAX actor steps
    DEVICE_AGENT_STEPS = 32             # actor steps per native call of that loop (1..64)
    DEVICE_DDPG = False                 # True (USE_DDPG, GAME = 'Pendulum-v0'): DEVICE_AGENTS environments step on the device under
                                        # DDPG, write their transitions into the replay ring in HBM, and the handle draws its own
                                        # train rows; no agent process, predictor, trainer or replay thread
    DEVICE_DDPG_UPDATES = 1             # train steps after each actor step of that loop (1..16)
    DEVICE_DDPG_EVAL_ENVS = 0           # > 0 (DEVICE_DDPG; at most 4096): this many evaluation environments beside the training ones.
                                        # The actor walks them without noise for a whole episode from fixed start states, one
                                        # launch, and the result goes to logs/<model>/eval.csv: the learned policy, where the
                                        # episode records are the exploring one's
    DEVICE_DDPG_EVAL_EVERY = 1000       # train steps between two evaluations (>= 1); one more before the first train step
    DEVICE_DDPG_EVAL_TARGET = False     # True: evaluate the target actor instead of the online one
    DEVICE_DDPG_NOISE = 'shared'        # 'shared': one step of the handle's noise process per actor step, added to every
                                        # environment's action; 'per_env' (DEVICE_DDPG with add_OUnoise): every environment has an
                                        # Ornstein-Uhlenbeck process of its own, as the reference's predicting processes had,
                                        # stepped inside the predict kernel
    DEVICE_DDPG_NOISE_RESET = False     # True: under 'per_env' an environment's process restarts at 0 when its episode ends
    # What "Pendulum-v0" means to the DEVICE_DDPG actors and evaluation episodes, option by option.  The defaults are the
    # fork's wrapper, EnvironmentPend.Environment, which the agent processes keep whatever these say; gym's own task is
    # ACTION_BOUND=clip TIME_LIMIT=truncate RESET_OBSERVATION=True REWARD_SCALE=1 REWARD_OFFSET=0.
    DEVICE_DDPG_ACTION_BOUND = 'wrap'   # 'wrap': an action beyond [-1, 1] turns around, 1.1 -> -0.9 (check_bounds with turnaround);
                                        # 'clip': it stops at the bound.  The ring keeps the action as predicted either way
    DEVICE_DDPG_TIME_LIMIT = 'terminal'     # 'terminal': the transition that reaches step 200 is done, y = r; 'truncate': the episode
                                        # ends and resets there all the same, but the row's done stays 0 and y bootstraps through
                                        # the observation before the reset
    DEVICE_DDPG_RESET_OBSERVATION = False   # True: after a reset the next transition starts from the reset state's observation;
                                        # False: from the last observation of the episode before, as the fork's wrapper leaves it
    DEVICE_DDPG_REWARD_SCALE = 0.005    # reward = -cost * DEVICE_DDPG_REWARD_SCALE + DEVICE_DDPG_REWARD_OFFSET (scale finite and > 0,
    DEVICE_DDPG_REWARD_OFFSET = -1.0    # offset finite).  DDPG_V_MIN / DDPG_V_MAX are fitted to the defaults and are the user's to set
                                        # for another reward: at (1, 0) the gamma = 0.99 return lies in about [-1650, 0]


VECTOR_GAMES = ('Pendulum-v0', 'CartPole-v0')      # games whose state is a vector (Server.py:35-43 of the reference)
VECTOR_GAME_CONTINUOUS = {'Pendulum-v0': True, 'CartPole-v0': False}   # ... and which of them has a continuous action space


def vector_game():
    return Config.GAME in VECTOR_GAMES


def discrete_vector_game():
    return vector_game() and not VECTOR_GAME_CONTINUOUS[Config.GAME]


def resolve_action_space(explicit=()):
    """DISCRATE_INPUT = not CONTINUOUS_INPUT, as the reference's Server.py:36-38 sets it.  `explicit`: the keys the command
    line gave.  DISCRATE_INPUT given alone decides CONTINUOUS_INPUT; both given and contradictory (the same value) raise.
    GAME = 'Pendulum-v0' sets CONTINUOUS_INPUT = True, as the reference's Server.py:35-38 does; a command line that asks
    for the discrete head with it raises.  GAME = 'CartPole-v0' sets CONTINUOUS_INPUT = False (Server.py:40-43) and raises
    on a command line that asks for the continuous head; DENSE_STACK is checked with it."""
    if discrete_vector_game():
        if ("CONTINUOUS_INPUT" in explicit and Config.CONTINUOUS_INPUT) or \
                ("DISCRATE_INPUT" in explicit and not Config.DISCRATE_INPUT):
            raise ValueError("GAME=%s has a discrete action space: CONTINUOUS_INPUT=%r / DISCRATE_INPUT=%r contradict it"
                             % (Config.GAME, Config.CONTINUOUS_INPUT, Config.DISCRATE_INPUT))
        if Config.DENSE_STACK not in ('fork', 'chained'):
            raise ValueError("DENSE_STACK=%r: 'fork' or 'chained'" % (Config.DENSE_STACK,))
        if Config.DUAL_RMSPROP:
            raise ValueError("DUAL_RMSPROP with GAME=%s is not supported" % Config.GAME)
        Config.CONTINUOUS_INPUT = False
        Config.DISCRATE_INPUT = True
        return
    if vector_game():
        if ("CONTINUOUS_INPUT" in explicit and not Config.CONTINUOUS_INPUT) or \
                ("DISCRATE_INPUT" in explicit and Config.DISCRATE_INPUT):
            raise ValueError("GAME=%s has a continuous action space: CONTINUOUS_INPUT=%r / DISCRATE_INPUT=%r contradict it"
                             % (Config.GAME, Config.CONTINUOUS_INPUT, Config.DISCRATE_INPUT))
        Config.CONTINUOUS_INPUT = True
        Config.DISCRATE_INPUT = False
        return
    if "DISCRATE_INPUT" in explicit and "CONTINUOUS_INPUT" in explicit:
        if bool(Config.DISCRATE_INPUT) == bool(Config.CONTINUOUS_INPUT):
            raise ValueError("DISCRATE_INPUT=%r contradicts CONTINUOUS_INPUT=%r" % (Config.DISCRATE_INPUT, Config.CONTINUOUS_INPUT))
    elif "DISCRATE_INPUT" in explicit:
        Config.CONTINUOUS_INPUT = not Config.DISCRATE_INPUT
    Config.DISCRATE_INPUT = not Config.CONTINUOUS_INPUT


def resolve_ddpg(explicit=(), num_actions=None):
    """What USE_DDPG implies (the reference's Config.py:160-178) and what it cannot be combined with here.  Call after
    resolve_action_space.  Without USE_DDPG nothing changes.  num_actions: the game's, where the caller knows it (DDPG_SOFT's
    head limit; NetworkDDPG.Network checks it too)."""
    if not Config.USE_DDPG:
        if Config.PRIORITIZED_REPLAY:
            raise ValueError("PRIORITIZED_REPLAY needs USE_DDPG: only the DDPG handle keeps a replay memory")
        if Config.DDPG_TWIN:
            raise ValueError("DDPG_TWIN needs USE_DDPG: the twin critics are the DDPG handle's")
        if Config.DDPG_DISTRIBUTIONAL:
            raise ValueError("DDPG_DISTRIBUTIONAL needs USE_DDPG: the distributional critic is the DDPG handle's")
        if Config.DDPG_POPART:
            raise ValueError("DDPG_POPART needs USE_DDPG: the normalised critic is the DDPG handle's")
        if Config.DDPG_SOFT:
            raise ValueError("DDPG_SOFT needs USE_DDPG: the soft actor-critic is the DDPG handle's")
        _resolve_nstep()
        return
    if not Config.CONTINUOUS_INPUT:
        raise ValueError("USE_DDPG needs a continuous action space (CONTINUOUS_INPUT); GAME=%s is discrete" % Config.GAME)
    if not vector_game():
        raise ValueError("USE_DDPG on an image game is not supported: the DDPG networks read vector states (GAME=Pendulum-v0)")
    for key, bad in (("DUAL_RMSPROP", True), ("HOGWILD", True), ("add_uncertainity", True)):
        if getattr(Config, key) == bad:
            raise ValueError("USE_DDPG with %s=%r is not supported" % (key, bad))
    if int(os.environ.get("WORLD_SIZE", "1") or 1) > 1:
        raise ValueError("USE_DDPG with WORLD_SIZE > 1 is not supported")
    if Config.FRONTEND == 'device':
        raise ValueError("USE_DDPG with FRONTEND='device' is not supported")
    if Config.DDPG_CRITIC_LOSS not in ('fork', 'paired'):
        raise ValueError("DDPG_CRITIC_LOSS=%r: 'fork' or 'paired'" % (Config.DDPG_CRITIC_LOSS,))
    if Config.TRAINING_MIN_BATCH_SIZE < 1:
        raise ValueError("USE_DDPG samples TRAINING_MIN_BATCH_SIZE rows per train step; the default 0 would train on empty "
                         "batches, as it does in the reference.  Set it, e.g. TRAINING_MIN_BATCH_SIZE=64")
    if Config.REPLAY_BUFFER_SIZE <= Config.TRAINING_MIN_BATCH_SIZE:
        raise ValueError("REPLAY_BUFFER_SIZE must exceed TRAINING_MIN_BATCH_SIZE: a batch is sampled only from more rows than it holds")
    if Config.PRIORITIZED_REPLAY:
        if Config.DDPG_CRITIC_LOSS != 'paired':
            raise ValueError("PRIORITIZED_REPLAY with DDPG_CRITIC_LOSS=%r is not supported: under the fork's loss the critic "
                             "regresses on the batch mean of y and a row has no TD error of its own.  Set "
                             "DDPG_CRITIC_LOSS=paired" % (Config.DDPG_CRITIC_LOSS,))
        if Config.REPLAY_BUFFER_SIZE > 1048576:
            raise ValueError("PRIORITIZED_REPLAY covers at most 1048576 rows (1024 chunks of 1024): REPLAY_BUFFER_SIZE=%d"
                             % Config.REPLAY_BUFFER_SIZE)
        if not 0.0 <= Config.PRIORITIZED_REPLAY_ALPHA <= 1.0:
            raise ValueError("PRIORITIZED_REPLAY_ALPHA=%r outside [0, 1]" % (Config.PRIORITIZED_REPLAY_ALPHA,))
        if not Config.PRIORITIZED_REPLAY_EPS > 0.0:
            raise ValueError("PRIORITIZED_REPLAY_EPS=%r: a number > 0" % (Config.PRIORITIZED_REPLAY_EPS,))
        if Config.PRIORITIZED_REPLAY_BETA_START < 0.0 or Config.PRIORITIZED_REPLAY_BETA_END < 0.0:
            raise ValueError("PRIORITIZED_REPLAY_BETA_START / _END = %r / %r: exponents >= 0"
                             % (Config.PRIORITIZED_REPLAY_BETA_START, Config.PRIORITIZED_REPLAY_BETA_END))
    if Config.DDPG_TWIN:
        if Config.DDPG_CRITIC_LOSS != 'paired':
            raise ValueError("DDPG_TWIN with DDPG_CRITIC_LOSS=%r is not supported: under the fork's loss the critics regress on "
                             "the batch mean of y and a row has no target of its own.  Set DDPG_CRITIC_LOSS=paired"
                             % (Config.DDPG_CRITIC_LOSS,))
        if not 1 <= int(Config.DDPG_POLICY_DELAY) <= 16:
            raise ValueError("DDPG_POLICY_DELAY=%r: a policy step every 1 to 16 train steps" % (Config.DDPG_POLICY_DELAY,))
        if not Config.DDPG_TARGET_NOISE >= 0.0 or not Config.DDPG_TARGET_NOISE_CLIP >= 0.0:
            raise ValueError("DDPG_TARGET_NOISE / _CLIP = %r / %r: numbers >= 0"
                             % (Config.DDPG_TARGET_NOISE, Config.DDPG_TARGET_NOISE_CLIP))
    if Config.DDPG_DISTRIBUTIONAL:
        if Config.DDPG_CRITIC_LOSS != 'paired':
            raise ValueError("DDPG_DISTRIBUTIONAL with DDPG_CRITIC_LOSS=%r is not supported: under the fork's loss a row has no "
                             "target of its own.  Set DDPG_CRITIC_LOSS=paired" % (Config.DDPG_CRITIC_LOSS,))
        if Config.DDPG_TWIN:
            raise ValueError("DDPG_DISTRIBUTIONAL with DDPG_TWIN is not supported: two distributions have no smaller one")
        n = Config.DDPG_ATOMS
        if isinstance(n, bool) or n != int(n) or not 2 <= int(n) <= 64:
            raise ValueError("DDPG_ATOMS=%r: a whole number of atoms from 2 to 64" % (n,))
        if not Config.DDPG_V_MIN < Config.DDPG_V_MAX:
            raise ValueError("DDPG_V_MIN / DDPG_V_MAX = %r / %r: the support's smaller end first"
                             % (Config.DDPG_V_MIN, Config.DDPG_V_MAX))
    if Config.DDPG_POPART:
        if Config.DDPG_CRITIC_LOSS != 'paired':
            raise ValueError("DDPG_POPART with DDPG_CRITIC_LOSS=%r is not supported: under the fork's loss the critic regresses on "
                             "the batch mean of y and a row has no target of its own to normalise.  Set DDPG_CRITIC_LOSS=paired"
                             % (Config.DDPG_CRITIC_LOSS,))
        if Config.DDPG_TWIN:
            raise ValueError("DDPG_POPART with DDPG_TWIN is not supported: the statistics normalise one scalar critic")
        if Config.DDPG_DISTRIBUTIONAL:
            raise ValueError("DDPG_POPART with DDPG_DISTRIBUTIONAL is not supported: the support fixes the returns' scale")
        beta, lo, hi = Config.DDPG_POPART_BETA, Config.DDPG_POPART_SIGMA_MIN, Config.DDPG_POPART_SIGMA_MAX
        if isinstance(beta, bool) or not 0.0 <= beta <= 1.0:
            raise ValueError("DDPG_POPART_BETA=%r outside [0, 1]" % (beta,))
        if isinstance(lo, bool) or isinstance(hi, bool) or not 0.0 < lo < hi < float("inf"):
            raise ValueError("DDPG_POPART_SIGMA_MIN / _MAX = %r / %r: two finite numbers, 0 < the first < the second" % (lo, hi))
    if Config.DDPG_SOFT:
        _resolve_soft(num_actions)
    _resolve_nstep()
    Config.USE_REPLAY_MEMORY = True
    Config.DISCOUNTING = False


def _resolve_soft(num_actions=None):
    """DDPG_SOFT on USE_DDPG.  num_actions: the game's, where the caller knows it (NetworkDDPG.Network does)."""
    if not Config.DDPG_TWIN:
        raise ValueError("DDPG_SOFT needs DDPG_TWIN: the soft actor-critic trains both critics on the smaller target value")
    if num_actions is not None and int(num_actions) > 16:
        raise ValueError("DDPG_SOFT with num_actions=%d is not supported: the Gaussian head has 2 x num_actions <= 32 columns"
                         % int(num_actions))
    alpha, rate, ent = Config.DDPG_SOFT_ALPHA, Config.DDPG_SOFT_ALPHA_LR, Config.DDPG_SOFT_TARGET_ENTROPY
    lo, hi = Config.DDPG_SOFT_LOG_STD_MIN, Config.DDPG_SOFT_LOG_STD_MAX
    if not _finite_number(alpha) or not alpha > 0:
        raise ValueError("DDPG_SOFT_ALPHA=%r: a finite number above 0" % (alpha,))
    if not _finite_number(rate) or rate < 0:
        raise ValueError("DDPG_SOFT_ALPHA_LR=%r: a finite factor >= 0" % (rate,))
    if ent is not None and not _finite_number(ent):
        raise ValueError("DDPG_SOFT_TARGET_ENTROPY=%r: None (-num_actions) or a finite number" % (ent,))
    if not _finite_number(lo) or not _finite_number(hi) or not lo < hi:
        raise ValueError("DDPG_SOFT_LOG_STD_MIN / _MAX = %r / %r: two finite numbers, the first the smaller" % (lo, hi))


def _resolve_nstep():
    """DDPG_NSTEP: 1 changes nothing anywhere; more needs the device actors of a DDPG handle."""
    n = Config.DDPG_NSTEP
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= 16:
        raise ValueError("DDPG_NSTEP=%r: a whole number of steps from 1 to 16" % (n,))
    if n == 1:
        return
    if not Config.USE_DDPG:
        raise ValueError("DDPG_NSTEP=%d needs USE_DDPG: the n-step returns are the DDPG handle's" % n)
    if not getattr(Config, "DEVICE_DDPG", False):
        raise ValueError("DDPG_NSTEP=%d needs DEVICE_DDPG: the n-step sum is formed in a per-environment window on the device.  "
                         "The agent processes ship rollouts cut at TIME_MAX with a repeated first row, and no window spans "
                         "them; the host path stays one-step" % n)
    if not Config.DDPG_FUTURE_REWARD_CALC:
        raise ValueError("DDPG_NSTEP=%d with DDPG_FUTURE_REWARD_CALC=False is not supported: y = r reads no discount" % n)


def _resolve_device_ddpg(n, pendulum):
    """DEVICE_AGENTS = n > 0 with DEVICE_DDPG.  DISCOUNTING, RETURN_MODE, USE_INTERMEDIATE_REWARD and TIME_MAX are
    not looked at: resolve_ddpg sets DISCOUNTING = False, and returns and rollout cuts play no part in a ring of transitions."""
    if not Config.USE_DDPG:
        raise ValueError("DEVICE_DDPG needs USE_DDPG: it puts the DDPG actors, replay writes and draws on the device")
    if Config.GAME != 'Pendulum-v0':
        raise ValueError("DEVICE_DDPG with GAME=%s is not supported: the device steps Pendulum-v0 under DDPG" % Config.GAME)
    if pendulum:
        raise ValueError("DEVICE_DDPG with DEVICE_PENDULUM is not supported: DEVICE_PENDULUM names the actor-critic regime "
                         "(lockstep rollouts), DEVICE_DDPG the replay regime; set one of them")
    if n > 4096:
        raise ValueError("DEVICE_AGENTS=%d with DEVICE_DDPG: at most 4096 environments, the DDPG handle's max_batch limit" % n)
    if n > Config.REPLAY_BUFFER_SIZE:
        raise ValueError("DEVICE_AGENTS=%d exceeds REPLAY_BUFFER_SIZE=%d: one actor step's transitions must fit the ring"
                         % (n, Config.REPLAY_BUFFER_SIZE))
    if not 1 <= int(Config.DEVICE_DDPG_UPDATES) <= 16:
        raise ValueError("DEVICE_DDPG_UPDATES=%r: 1 to 16 train steps per actor step" % (Config.DEVICE_DDPG_UPDATES,))
    if Config.PLAY_MODE:
        raise ValueError("DEVICE_AGENTS with PLAY_MODE is not supported: the device actors train as they step")
    if Config.DYNAMIC_SETTINGS:
        raise ValueError("DEVICE_AGENTS with DYNAMIC_SETTINGS is not supported: there are no workers to add or remove")
    if int(os.environ.get("WORLD_SIZE", "1") or 1) > 1:
        raise ValueError("DEVICE_AGENTS with WORLD_SIZE > 1 is not supported")
    if not 1 <= int(Config.DEVICE_AGENT_STEPS) <= 64:
        raise ValueError("DEVICE_AGENT_STEPS=%r: 1 to 64 actor steps per call" % (Config.DEVICE_AGENT_STEPS,))
    e = Config.DEVICE_DDPG_EVAL_ENVS
    if isinstance(e, bool) or not isinstance(e, int) or not 0 <= e <= 4096:
        raise ValueError("DEVICE_DDPG_EVAL_ENVS=%r: 0 (off) or 1 to 4096 evaluation environments" % (e,))
    if e:                                   # (off: the two keys beside it are not looked at)
        k = Config.DEVICE_DDPG_EVAL_EVERY
        if isinstance(k, bool) or not isinstance(k, int) or k < 1:
            raise ValueError("DEVICE_DDPG_EVAL_EVERY=%r: a whole number of train steps >= 1" % (k,))
        if not isinstance(Config.DEVICE_DDPG_EVAL_TARGET, bool):
            raise ValueError("DEVICE_DDPG_EVAL_TARGET=%r: True or False" % (Config.DEVICE_DDPG_EVAL_TARGET,))
    mode = Config.DEVICE_DDPG_NOISE
    if mode not in ('shared', 'per_env'):
        raise ValueError("DEVICE_DDPG_NOISE=%r: 'shared' or 'per_env'" % (mode,))
    if mode == 'per_env' and not Config.add_OUnoise:
        raise ValueError("DEVICE_DDPG_NOISE='per_env' with add_OUnoise=%r is not supported: there is no noise process to give "
                         "each environment" % (Config.add_OUnoise,))
    if mode == 'per_env' and Config.DDPG_SOFT:
        raise ValueError("DEVICE_DDPG_NOISE='per_env' with DDPG_SOFT is not supported: the policy's own sampling is already per "
                         "environment")
    if not isinstance(Config.DEVICE_DDPG_NOISE_RESET, bool):
        raise ValueError("DEVICE_DDPG_NOISE_RESET=%r: True or False" % (Config.DEVICE_DDPG_NOISE_RESET,))
    _resolve_device_ddpg_task()


# The five keys of the device actors' task and their defaults: the fork's wrapper.
DEVICE_DDPG_TASK_DEFAULTS = (("DEVICE_DDPG_ACTION_BOUND", 'wrap'), ("DEVICE_DDPG_TIME_LIMIT", 'terminal'),
                             ("DEVICE_DDPG_RESET_OBSERVATION", False), ("DEVICE_DDPG_REWARD_SCALE", 0.005),
                             ("DEVICE_DDPG_REWARD_OFFSET", -1.0))


def _finite_number(v):
    return not isinstance(v, bool) and isinstance(v, (int, float)) and math.isfinite(v)


def _resolve_device_ddpg_task():
    if Config.DEVICE_DDPG_ACTION_BOUND not in ('wrap', 'clip'):
        raise ValueError("DEVICE_DDPG_ACTION_BOUND=%r: 'wrap' or 'clip'" % (Config.DEVICE_DDPG_ACTION_BOUND,))
    if Config.DEVICE_DDPG_TIME_LIMIT not in ('terminal', 'truncate'):
        raise ValueError("DEVICE_DDPG_TIME_LIMIT=%r: 'terminal' or 'truncate'" % (Config.DEVICE_DDPG_TIME_LIMIT,))
    if not isinstance(Config.DEVICE_DDPG_RESET_OBSERVATION, bool):
        raise ValueError("DEVICE_DDPG_RESET_OBSERVATION=%r: True or False" % (Config.DEVICE_DDPG_RESET_OBSERVATION,))
    if not _finite_number(Config.DEVICE_DDPG_REWARD_SCALE) or not Config.DEVICE_DDPG_REWARD_SCALE > 0:
        raise ValueError("DEVICE_DDPG_REWARD_SCALE=%r: a finite number above 0" % (Config.DEVICE_DDPG_REWARD_SCALE,))
    if not _finite_number(Config.DEVICE_DDPG_REWARD_OFFSET):
        raise ValueError("DEVICE_DDPG_REWARD_OFFSET=%r: a finite number" % (Config.DEVICE_DDPG_REWARD_OFFSET,))


def _refuse_task_without_device_ddpg():
    """A non-default task key asks for the task of the DDPG handle's device actors."""
    for key, default in DEVICE_DDPG_TASK_DEFAULTS:
        value = getattr(Config, key, default)
        if value != default:                  # the comparison NetworkDDPG makes before it attaches a task
            raise ValueError("%s=%r needs DEVICE_DDPG (with DEVICE_AGENTS > 0): the task is that of the DDPG actors stepped on "
                             "the device; the agent processes keep the fork's wrapper" % (key, value))


def _refuse_eval_without_device_ddpg():
    """DEVICE_DDPG_EVAL_ENVS asks for evaluation episodes of the DDPG handle's device regime."""
    if getattr(Config, "DEVICE_DDPG_EVAL_ENVS", 0):
        raise ValueError("DEVICE_DDPG_EVAL_ENVS=%r needs DEVICE_DDPG (with DEVICE_AGENTS > 0): the evaluation episodes are run by "
                         "the loop that steps the DDPG actors on the device" % (Config.DEVICE_DDPG_EVAL_ENVS,))


def _refuse_env_noise_without_device_ddpg():
    """DEVICE_DDPG_NOISE = 'per_env'  asks for the noise of the DDPG handle's device actors."""
    if getattr(Config, "DEVICE_DDPG_NOISE", 'shared') == 'per_env':
        raise ValueError("DEVICE_DDPG_NOISE='per_env' needs DEVICE_DDPG (with DEVICE_AGENTS > 0): the per-environment noise is "
                         "that of the DDPG actors stepped on the device")


def resolve_device_agents(explicit=()):
    """What DEVICE_AGENTS > 0 cannot be combined with.  Call after resolve_action_space and resolve_ddpg.  With
    DEVICE_AGENTS = 0 nothing is checked and nothing changes, except that DEVICE_DDPG, which asks for them, raises, and so
    do DEVICE_DDPG_EVAL_ENVS > 0, DEVICE_DDPG_NOISE = 'per_env' and a non-default key of the task, which ask for DEVICE_DDPG."""
    n = int(Config.DEVICE_AGENTS)
    if n == 0:
        if getattr(Config, "DEVICE_DDPG", False):
            raise ValueError("DEVICE_DDPG needs DEVICE_AGENTS > 0: the number of environments on the device")
        _refuse_eval_without_device_ddpg()
        _refuse_env_noise_without_device_ddpg()
        _refuse_task_without_device_ddpg()
        return
    if n < 0:
        raise ValueError("DEVICE_AGENTS=%d: 0 (off) or the number of environments on the device" % n)
    pendulum = bool(getattr(Config, "DEVICE_PENDULUM", False))
    if getattr(Config, "DEVICE_DDPG", False):
        _resolve_device_ddpg(n, pendulum)
        return
    _refuse_eval_without_device_ddpg()
    _refuse_env_noise_without_device_ddpg()
    _refuse_task_without_device_ddpg()
    if Config.USE_DDPG:
        raise ValueError("DEVICE_AGENTS with USE_DDPG is not supported: the device actors step CartPole-v0 only, or "
                         "Pendulum-v0 under the actor-critic network (DEVICE_PENDULUM); under DDPG they need DEVICE_DDPG=True")
    if pendulum and Config.GAME != 'Pendulum-v0':
        raise ValueError("DEVICE_PENDULUM with GAME=%s is not supported: it asks for Pendulum-v0 environments on the device"
                         % Config.GAME)
    if Config.GAME != 'CartPole-v0' and not pendulum:
        raise ValueError("DEVICE_AGENTS with GAME=%s is not supported: the device actors step CartPole-v0 only, and "
                         "Pendulum-v0 with DEVICE_PENDULUM=True, where they run in lockstep (the image games keep their agent "
                         "processes)" % Config.GAME)
    if Config.RETURN_MODE != 'fork':
        raise ValueError("DEVICE_AGENTS with RETURN_MODE=%r is not supported: the device computes the fork's returns" % Config.RETURN_MODE)
    if not Config.DISCOUNTING or Config.USE_INTERMEDIATE_REWARD:
        raise ValueError("DEVICE_AGENTS computes the fork's returns with DISCOUNTING and without USE_INTERMEDIATE_REWARD only")
    if Config.PLAY_MODE:
        raise ValueError("DEVICE_AGENTS with PLAY_MODE is not supported: the device actors train as they step")
    if Config.DYNAMIC_SETTINGS:
        raise ValueError("DEVICE_AGENTS with DYNAMIC_SETTINGS is not supported: there are no workers to add or remove")
    if int(os.environ.get("WORLD_SIZE", "1") or 1) > 1:
        raise ValueError("DEVICE_AGENTS with WORLD_SIZE > 1 is not supported")
    if Config.TIME_MAX < 1:
        raise ValueError("DEVICE_AGENTS needs TIME_MAX >= 1")
    if not 1 <= int(Config.DEVICE_AGENT_STEPS) <= 64:
        raise ValueError("DEVICE_AGENT_STEPS=%r: 1 to 64 actor steps per call" % (Config.DEVICE_AGENT_STEPS,))
    rows = n * (Config.TIME_MAX + 1)
    if rows > 65536:
        raise ValueError("DEVICE_AGENTS=%d x (TIME_MAX + 1 = %d) = %d rows exceed the 65536 rows a train call of the network "
                         "can take (its max_batch)" % (n, Config.TIME_MAX + 1, rows))
