"""Regenerates tests/golden/replay_buffer.json.  Run in the BUILD container only (`python tests/golden/make_golden_ddpg.py`);
the reference does not exist on the GPU box.

The reference's ReplayBuffer (replay_buffer.py; it needs numpy and the standard library only) is imported and RUN: for a few
(capacity, adds, batch) triples rows tagged with their running number are added in rollout-sized chunks, and after every
chunk a batch is sampled whenever the buffer holds more than `batch` rows (ThreadReplay.py:52-55 samples before it adds;
the order of the two inside a pass does not change what a sample of a given buffer is).  Recorded per sample: the rows
ever added at that moment, the tags drawn, and their positions in the deque (0 = oldest); per case the tags left at the
end, oldest first (the eviction order).  Data only: inputs and recorded outputs.
"""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/ga3c"
SEED = 12345                                    # Config.REPLAY_BUFFER_RANDOM_SEED
CASES = [(50, 170, 8, 6), (64, 64, 16, 6), (1000, 400, 64, 6), (7, 40, 3, 5)]     # capacity, adds, batch, chunk


def main():
    sys.path.insert(0, REF)
    from replay_buffer import ReplayBuffer      # reference module
    cases = []
    for capacity, adds, batch, chunk in CASES:
        buf = ReplayBuffer(capacity, SEED)
        total, samples = 0, []
        while total < adds:
            n = min(chunk, adds - total)
            for _ in range(n):
                buf.add(total, 0.0, 0.0, False, total)
                total += 1
            if buf.size() > batch:
                tags = [int(t) for t in buf.sample_batch(batch)[0]]
                oldest = int(buf.buffer[0][0])
                samples.append({"total": total, "tags": tags, "positions": [t - oldest for t in tags]})
        cases.append({"capacity": capacity, "adds": adds, "batch": batch, "chunk": chunk, "seed": SEED, "samples": samples,
                      "final_size": int(buf.size()), "final_tags": [int(e[0]) for e in buf.buffer]})
    with open(os.path.join(HERE, "replay_buffer.json"), "w") as f:
        json.dump({"cases": cases}, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
