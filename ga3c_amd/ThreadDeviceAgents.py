"""Config.DEVICE_AGENTS > 0: the one worker thread of a server whose agents live on the device.  It stands
for every ProcessAgent, ThreadPredictor and ThreadTrainer at once: the model steps DEVICE_AGENTS environments (CartPole-v0,
or Pendulum-v0 with DEVICE_PENDULUM), predicts for them and trains on the rollouts they cut, all in HBM
(NetworkVP_vecnet.DeviceActors.actors_run), and this loop
only asks for the next DEVICE_AGENT_STEPS steps, hands the finished episodes to the statistics process in the order they
finished and keeps the server's counters.  learning_rate and beta are the model's, which Server.main anneals.
With DEVICE_DDPG the model is NetworkDDPG.Network: the environments write transitions into its replay ring, it
trains on rows it draws itself (ThreadReplay is not started), and the ring's size goes to the status line.
With DEVICE_DDPG_EVAL_ENVS > 0 the loop also asks the model for a noise-free evaluation before the first train step
and whenever the train steps have passed a multiple of DEVICE_DDPG_EVAL_EVERY, and the model appends it to logs/<model>/eval.csv;
a model is asked for eval_* only then."""
import queue
from datetime import datetime
from threading import Thread

from Config import Config

EVAL_STEPS = 200                        # a whole Pendulum-v0 episode under its TimeLimit


class ThreadDeviceAgents(Thread):
    def __init__(self, server):
        super(ThreadDeviceAgents, self).__init__()
        self.daemon = True
        self.server = server
        self.exit_flag = False
        self.served = 0                 # predictions the actors took an action from
        self.agent_steps = 0
        self.episodes = 0
        self.evaluations = 0

    def run(self):
        try:
            self._run()
        except BaseException as e:   # noqa: BLE001
            self.server.worker_failed(type(self).__name__, e)

    def _log_episode(self, reward, length):
        """episode_log_q.put, looking at exit_flag while the statistics process is behind -> False when told to stop."""
        item = (datetime.now(), reward, length)
        while not self.exit_flag:
            try:
                self.server.stats.episode_log_q.put(item, timeout=Config.QUEUE_TIMEOUT_MS / 1000.0)
                return True
            except queue.Full:
                pass
        return False

    def _evaluate(self):
        """One evaluation of the model's actor as it stands, into eval.csv at the server's train step."""
        totals = self.server.model.eval_run(EVAL_STEPS, bool(Config.DEVICE_DDPG_EVAL_TARGET))
        self.server.model.log_eval(self.server.training_step, totals, EVAL_STEPS)
        self.evaluations += 1

    def _run(self):
        server, model = self.server, self.server.model
        n, chunk = int(Config.DEVICE_AGENTS), int(Config.DEVICE_AGENT_STEPS)
        evaluating = int(getattr(Config, "DEVICE_DDPG_EVAL_ENVS", 0)) > 0
        every = int(Config.DEVICE_DDPG_EVAL_EVERY) if evaluating else 0
        model.actors_create(n, Config.TIME_MAX, Config.DISCOUNT, Config.RANDOM_SEED)
        first = True
        try:
            if evaluating:
                model.eval_create(int(Config.DEVICE_DDPG_EVAL_ENVS), Config.RANDOM_SEED + 1)
                self._evaluate()                # a curve's point zero, before the first train step
                evaluated = server.training_step // every
            while not self.exit_flag:
                steps, calls, rows, _ = model.actors_run(chunk, train=bool(Config.TRAIN_MODELS))
                self.agent_steps += steps
                self.served += steps - (n if first else 0)      # an environment's first ever step is unpredicted
                first = False
                server.training_step += calls
                server.frame_counter += rows
                server.stats.training_count.value += calls
                if evaluating and server.training_step // every > evaluated:      # passed a multiple since the last one
                    evaluated = server.training_step // every
                    self._evaluate()
                if hasattr(model, "replay_size"):       # DEVICE_DDPG: the rows the replay ring holds
                    server.stats.replay_memory_size.value = model.replay_size()[0]
                for reward, length in model.actors_episodes():
                    if not self._log_episode(reward, length):
                        break                   # told to stop: the loop ends on exit_flag
                    self.episodes += 1
        except BaseException:
            for destroy in (("eval_destroy",) if evaluating else ()) + ("actors_destroy",):
                try:                    # the failure that ended the loop is the one to report, not what the clean-up makes of it
                    getattr(model, destroy)()
                except Exception:   # noqa: BLE001
                    pass
            raise
        if evaluating:
            model.eval_destroy()
        model.actors_destroy()
