"""Actor-side initial priorities (ofx_replay_capture_valued, include/ofx.h), restated in numpy for ONE arena.

The arithmetic is the device's: the targets in float32 in the operation order of ofx_dqn_targets (the product gamma * v
rounds on its own, then the sum with the reward; a done row never reads v), the errors e = previous value - target in
float32, the mass by tests/per_oracle.new_mass (p summed in float32, the power in float64: the device's powf is what a
2-ulp comparison checks).  A non-finite error gives the row the running maximum as it was BEFORE the lock-step; afterwards
the maximum is raised to the largest new mass formed from finite errors.

It is driven by what a test recorded per lock-step and ship: reward, done, has_row (a row completes: the ship plays and
has a previous observation), plays (the ship is selected and not latched), and the four values of ofx_policy_act."""
from collections import deque

import numpy as np

from tests import per_oracle

f32 = np.float32


def td_errors(reward, done, prev_q_sa, prev_p_sp, v_act, v_ptr, gamma):
    """(e1, e2) float32 of one completed row."""
    r, g = f32(reward), f32(gamma)
    with np.errstate(all="ignore"):
        if done:
            y1 = y2 = r
        else:
            y1 = f32(r + f32(g * f32(v_act)))
            y2 = f32(r + f32(g * f32(v_ptr)))
        return f32(f32(prev_q_sa) - y1), f32(f32(prev_p_sp) - y2)


class ArenaOracle:
    def __init__(self, n_ships, capacity, alpha, eps, gamma):
        self.M, self.alpha, self.eps, self.gamma = n_ships, alpha, eps, gamma
        self.mass = deque(maxlen=capacity)          # oldest first, like ofx_replay_priorities_host
        self.mmax = 1.0
        self.prev_q = np.zeros((n_ships, 2), f32)
        self.fallbacks = 0                          # rows that took the running maximum

    def capture_valued(self, reward, done, has_row, plays, q_sa, p_sp, v_act, v_ptr):
        before, raised = self.mmax, 0.0
        for i in range(self.M):                     # rows are appended in ship order
            if not has_row[i]:
                continue
            e1, e2 = td_errors(reward[i], done[i], self.prev_q[i, 0], self.prev_q[i, 1], v_act[i], v_ptr[i], self.gamma)
            if np.isfinite(e1) and np.isfinite(e2):
                m = per_oracle.new_mass(e1, e2, self.alpha, self.eps)
                raised = max(raised, m)
            else:
                m = before
                self.fallbacks += 1
            self.mass.append(m)
        if np.any(has_row):
            self.mmax = max(before, raised)
        for i in range(self.M):
            if plays[i]:
                self.prev_q[i] = (q_sa[i], p_sp[i])

    def capture_plain(self, has_row):
        """ofx_replay_capture on the same memory: every new row takes the running maximum, prev_q stays."""
        for i in range(self.M):
            if has_row[i]:
                self.mass.append(self.mmax)

    def reset(self):
        """An episode start clears has_prev on the device; the stale prev_q is simply never read (has_row is False until
        the ship has played again), so there is nothing to do here."""


def within_2ulp(got, want):
    """The rule of tests/test_prioritized_replay.py: |device float32 - float64 restatement| <= 2 ulp of the latter."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return got.shape == want.shape and bool((np.abs(got - want) <= 2 * np.spacing(want.astype(f32)).astype(np.float64)).all())
