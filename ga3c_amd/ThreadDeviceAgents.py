"""Config.DEVICE_AGENTS > 0: the one worker thread of a server whose agents live on the device.  It stands
for every ProcessAgent, ThreadPredictor and ThreadTrainer at once: the model steps DEVICE_AGENTS environments (CartPole-v0,
or Pendulum-v0 with DEVICE_PENDULUM), predicts for them and trains on the rollouts they cut, all in HBM
(NetworkVP_vecnet.DeviceActors.actors_run), and this loop
only asks for the next DEVICE_AGENT_STEPS steps, hands the finished episodes to the statistics process in the order they
finished and keeps the server's counters.  learning_rate and beta are the model's, which Server.main anneals.
With DEVICE_DDPG the model is NetworkDDPG.Network: the environments write transitions into its replay ring, it
trains on rows it draws itself (ThreadReplay is not started), and the ring's size goes to the status line."""
import queue
from datetime import datetime
from threading import Thread

from Config import Config


class ThreadDeviceAgents(Thread):
    def __init__(self, server):
        super(ThreadDeviceAgents, self).__init__()
        self.daemon = True
        self.server = server
        self.exit_flag = False
        self.served = 0                 # predictions the actors took an action from
        self.agent_steps = 0
        self.episodes = 0

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

    def _run(self):
        server, model = self.server, self.server.model
        n, chunk = int(Config.DEVICE_AGENTS), int(Config.DEVICE_AGENT_STEPS)
        model.actors_create(n, Config.TIME_MAX, Config.DISCOUNT, Config.RANDOM_SEED)
        first = True
        try:
            while not self.exit_flag:
                steps, calls, rows, _ = model.actors_run(chunk, train=bool(Config.TRAIN_MODELS))
                self.agent_steps += steps
                self.served += steps - (n if first else 0)      # an environment's first ever step is unpredicted
                first = False
                server.training_step += calls
                server.frame_counter += rows
                server.stats.training_count.value += calls
                if hasattr(model, "replay_size"):       # DEVICE_DDPG: the rows the replay ring holds
                    server.stats.replay_memory_size.value = model.replay_size()[0]
                for reward, length in model.actors_episodes():
                    if not self._log_episode(reward, length):
                        break                   # told to stop: the loop ends on exit_flag
                    self.episodes += 1
        except BaseException:
            try:                        # the failure that ended the loop is the one to report, not what the clean-up makes of it
                model.actors_destroy()
            except Exception:   # noqa: BLE001
                pass
            raise
        model.actors_destroy()
