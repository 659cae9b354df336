"""Replay thread (reference: ga3c/ThreadReplay.py:48-61 over replay_buffer.py:16-55), with the memory itself in HBM.

Each pass, as there: if fewer than REPLAY_MIN_QUEUE_SIZE batches are queued and the memory holds MORE than
TRAINING_MIN_BATCH_SIZE rows, sample TRAINING_MIN_BATCH_SIZE of them and queue the batch; then take ONE rollout from the
training queue (blocking) and append its rows.  The reference samples with random.sample(deque, k), which uses only the
deque's length and positions: random.Random(seed).sample(range(size), k) draws the same positions, and position j of the
deque is ring slot (oldest + j) mod capacity (tests/golden/replay_buffer.json).

What travels to a trainer is (slots int32[B], stamp): the ring slots and the number of rows ever added when they were
sampled.  The model's train_replay refuses a batch one of whose slots has been written since (StateLost; the server drops
and counts it), so a row is never trained on after it was overwritten; ring writes and train steps are ordered on the
handle's one stream, so a row is never read half written either.

Under Config.PRIORITIZED_REPLAY the thread draws nothing: under the same two rules it queues the token (None, total), and the
trainer that takes it calls the model's train_prioritized, which draws the rows on the device by their priorities at the
moment it trains.  No slot is named ahead of time, so no batch can be lost, and self.random is never used.

Rollout rows are `s | s2 | done | padding` in f32 (ProcessAgent._ship), returns carry the un-accumulated rewards
(DISCOUNTING = False).  With zero-copy intake the device reads the rows where they lie and the slot goes back to the agents
when replay_add_offsets returns, which is after the device has read them.  The thread holds one rollout at a time.
"""
import random
from threading import Thread

import numpy as np

from Config import Config


def ring_slots(positions, total, capacity):
    """Positions in the reference's deque (0 = oldest) -> slots of a ring that has had `total` rows appended."""
    oldest = total % capacity if total > capacity else 0
    return ((oldest + np.asarray(positions, np.int64)) % capacity).astype(np.int32)


def rollout_row_bytes(state_floats):
    """A DDPG rollout row: s[S] | s2[S] | done, f32, padded to a multiple of 16 bytes (32 at S = 3)."""
    return (8 * int(state_floats) + 4 + 15) // 16 * 16


class ThreadReplay(Thread):
    def __init__(self, server, transport=None):
        super(ThreadReplay, self).__init__()
        self.daemon = True
        self.server = server
        self.transport = transport if transport is not None else server.transport
        self.exit_flag = False
        self.random = random.Random(Config.REPLAY_BUFFER_RANDOM_SEED)     # random.seed(random_seed), replay_buffer.py:24
        self.size = 0               # rows held
        self.total = 0              # rows ever added
        self.capacity = int(getattr(server.model, "replay_capacity", Config.REPLAY_BUFFER_SIZE))
        self.batches = 0

    def update_stats(self):
        self.server.stats.replay_memory_size.value = self.size

    def run(self):
        try:
            self._run()
        except BaseException as e:   # noqa: BLE001
            report = getattr(self.server, "worker_failed", None)
            if report is None:
                raise
            report(type(self).__name__, e)

    def sample(self):
        """-> (slots, stamp) of one batch, or None while the memory does not hold MORE than a batch.  PRIORITIZED_REPLAY:
        (None, stamp), the device draws."""
        k = Config.TRAINING_MIN_BATCH_SIZE
        if not self.size > k:
            return None
        if Config.PRIORITIZED_REPLAY:
            return None, self.total
        return ring_slots(self.random.sample(range(self.size), k), self.total, self.capacity), self.total

    def add(self, slot):
        t, model = self.transport, self.server.model
        rows = t.rows(slot)
        states, returns, actions = t.rollout_views(slot)
        if getattr(self.server, "zero_copy", False):
            self.size, self.total = model.replay_add_offsets(t.rollout_row_offsets(slot, rows), returns[:rows], actions[:rows])
        else:
            S = int(self.server.state_dim[0])
            f = states[:rows].view(np.float32)
            self.size, self.total = model.replay_add(f[:, :S], actions[:rows], returns[:rows], f[:, 2 * S], f[:, S:2 * S])
        t.release(slot)

    def _run(self):
        t = self.transport
        while not self.exit_flag:
            if self.server.replay_q.qsize() < Config.REPLAY_MIN_QUEUE_SIZE:
                batch = self.sample()
                if batch is not None:
                    self.server.replay_q.put(batch)
                    self.batches += 1
            slot = -3
            while slot == -3 and not self.exit_flag:        # training_q.get(): blocking; the timeout only looks at exit_flag
                slot = t.pop_rollout(Config.QUEUE_TIMEOUT_MS)
            if slot < 0:
                return                                      # transport shut down (or told to stop)
            self.add(slot)
            self.update_stats()
