"""Oracle of the n-step returns of the DDPG device actors (Config.DDPG_NSTEP, ga3c_ddpg_nstep_*; the kernel is
ddpg_actors_nstep_kernel<PendulumBounded> of csrc/ga3c_ddpg.hip: the step is actor_step, which it shares with
ddpg_actors_step_kernel, and the window and the emitted row are its own), restated in numpy on top of ddpg_actors_oracle.Actors and Ring.

The rule, as a delay line.  c = 0, 1, 2, .. numbers the transitions an environment has made since its actors were created
(step(None) makes none; all environments step together, so c is one number).  Each environment keeps its last n transitions
(s_c, a_c as predicted, the f64 reward r_c, done_c, s2_c), transition c in window entry c mod n.
  * a step with c < n - 1 emits nothing;
  * every later step emits one row per environment, for the transition that began at u = c - n + 1:
      m = the smallest k in 1..n with done_{u+k-1} = 1, n if there is none
      R = sum_{k<m} g_k r_{u+k}, summed in f64 with ascending k from 0.0, g_0 = 1, g_{k+1} = g_k gamma64, gamma64 the f32
          gamma widened to f64; no fused multiply-add
      row = s_u | a_u | (f32) R | done_{u+m-1} | s2_{u+m-1},  disc = (f32) g_m
    so the last n - 1 transitions of an episode leave with shortened horizons and done = 1 while the next episode has nothing of
    its own to emit, nothing is summed across an episode's end, and the last n - 1 transitions before a destroy never leave.
  * at n = 1 the row is ddpg_actors_oracle's and disc is gamma, bit for bit: 0.0 + 1.0 r = r, 1.0 gamma64 = gamma64.
The rows go to ring slot (rows ever added + i) mod capacity in environment order, disc beside them by slot.

brute_force states the same rows per episode, without a window: for every transition j of an episode of L transitions, the
return over the next min(n, L - j) of them.  tests/test_nstep_cpu.py holds the delay line to it.

A train step's target on ring rows is y = fmaf(disc[slot], q', R) on rows that are not done: ddpg_oracle.targets / train_step,
per_oracle.train_step and td3_oracle.targets take the array of the rows' discounts in gamma's place and broadcast it.
"""
import numpy as np

import ddpg_actors_oracle as do


def gamma64(gamma):
    return float(np.float32(gamma))


def nstep_row(entries, gamma):
    """entries: the transitions (s, a, r f64, done, s2) from u on, oldest first, at most n of them -> (row, disc)."""
    g64 = gamma64(gamma)
    R, g, last = 0.0, 1.0, None
    for t in entries:
        R = R + g * float(t[2])
        g = g * g64
        last = t
        if t[3]:
            break
    s, a = entries[0][0], entries[0][1]
    return (s, a, np.float32(R), np.float32(1.0 if last[3] else 0.0), last[4]), np.float32(g)


class DelayLine:
    """The windows of N environments.  push(transitions) with one (s, a, r f64, done, s2) per environment -> None on a silent
    step, else [(row, disc)] in environment order."""

    def __init__(self, n_env, n, gamma):
        assert 1 <= n <= 16
        self.n, self.gamma, self.count = int(n), gamma, 0
        self.win = [[None] * self.n for _ in range(n_env)]

    def push(self, transitions):
        n, c = self.n, self.count
        assert len(transitions) == len(self.win)
        for w, t in zip(self.win, transitions):
            w[c % n] = t
        self.count += 1
        if c < n - 1:
            return None
        oldest = (c + 1) % n
        return [nstep_row([w[(oldest + k) % n] for k in range(n)], self.gamma) for w in self.win]


def brute_force(transitions, n, gamma):
    """One environment's whole stream of transitions, in step order -> [(u, row, disc)] by u: per episode (ended by done = 1; a
    last one may be unfinished), transition j of L has the horizon min(n, L - j).  Transition u leaves on step u + n - 1, so of a
    stream of T transitions those with u + n <= T have left; in an unfinished episode these are the ones with a full horizon."""
    out, start, T = [], 0, len(transitions)
    while start < T:
        end = start
        while end < T and not transitions[end][3]:
            end += 1
        L = (end - start + 1) if end < T else (T - start)
        for j in range(L):
            m = min(n, L - j)
            if start + j + n > T:           # it leaves on step u + n - 1, which the stream has not reached
                continue
            row, disc = nstep_row(transitions[start + j:start + j + m], gamma)
            out.append((start + j, row, disc))
        start += L
    return out


class Ring(do.Ring):
    """ddpg_actors_oracle.Ring with the discount of the row in each slot: gamma until an n-step row is written."""

    def __init__(self, capacity, prioritized=False, gamma=0.99):
        super().__init__(capacity, prioritized)
        self.disc = np.full(self.capacity, np.float32(gamma), np.float32)

    def add(self, rows, discs):
        slots = super().add(rows)
        for slot, d in zip(slots, discs):
            self.disc[slot] = np.float32(d)
        return slots


class Actors(do.Actors):
    """ddpg_actors_oracle.Actors whose transitions pass through a DelayLine.  step(actions, s2=None) -> (emitted [(row, disc)]
    in environment order, empty on a silent step; episode records; the per-environment outputs).  s2 [N, S]: the observations
    to keep as the transitions' s2 in the oracle's place (the device's own, whose cos and sin are its library's)."""

    def __init__(self, n_env, seed, n, gamma):
        super().__init__(n_env, seed)
        self.line = DelayLine(n_env, n, gamma)

    def step(self, actions=None, rewards=None, s2=None):
        rows, episodes, outs = super().step(actions, rewards)
        if not rows:
            return [], episodes, outs
        trans = [(row[0], row[1], np.float64(out["reward"]), bool(out["done"]), row[4] if s2 is None else np.array(s2[i], np.float32))
                 for i, (row, out) in enumerate(zip(rows, outs))]
        return self.line.push(trans) or [], episodes, outs
