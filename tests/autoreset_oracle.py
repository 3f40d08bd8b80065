"""Per-arena episodes (ofx_restart_finished, include/ofx.h) restated on the CPU oracle: every arena keeps its own clock,
episode counter and `dead_once` marks, restarts on pyoracle.reset_draws(cfg, seed, global arena, arena_episode) through
Arena.restart, and banks into the [G][M+2] sums.  The GPU tests compare against this model lock-step by lock-step;
tests/test_auto_reset.py asserts, on the model alone, that the scenarios exercise what they must."""
import numpy as np

from oracle import pyoracle
from tests import repeat_oracle as ro

N, STEPS, MAX_TICKS = 5, 120, 40                   # 5 arenas: not a multiple of the 4 arenas of a block
SCENARIOS = {                                      # the two scenarios of the issue, and the clock alone
    "M8": dict(seed=777, m=8, selected=(0, 3)),
    "M13": dict(seed=12345, m=13, selected=(0, 12)),
    "nobody": dict(seed=777, m=8, selected=()),
}


def behaviours(m):
    """repeat_oracle's line-up repeated to m ships."""
    return [ro.BEHAVIOURS[i % len(ro.BEHAVIOURS)] for i in range(m)]


class Model:
    """n arenas (global ids arena_base .. arena_base + n - 1) under the restart rule.  mask: bool [n][m], the selected
    ships; group: int [n] or None (one group)."""

    def __init__(self, seed, n, m, mask, max_ticks, arena_base=0, group=None, n_groups=1):
        self.seed, self.n, self.m, self.base, self.max_ticks = seed, n, m, arena_base, max_ticks
        self.mask = np.asarray(mask, bool).reshape(n, m)
        self.group, self.n_groups = group, n_groups
        self.beh = np.array([ro.BOT[b] for b in behaviours(m)], np.int32)
        self.arenas = []
        for a in range(n):
            o = pyoracle.Arena(cfg=pyoracle.default_cfg(m, **ro.REWARDS))
            o.spawn(pyoracle.reset_draws(o.cfg, seed, arena_base + a, 0))
            self.arenas.append(o)
        self.time = np.zeros(n, np.int32)
        self.arena_episode = np.zeros(n, np.uint32)
        self.dead_once = np.zeros((n, m), np.uint8)
        self.restarted = np.zeros(n, np.uint8)
        self.died = np.zeros(n, np.uint8)          # the arenas the last call restarted because their ships were finished
        self.sums = np.zeros((n_groups, m + 2), np.int64)
        self.by_death = self.by_clock = self.zero_draws = self.waiting = 0

    def restart_finished(self):
        """One call of the rule; returns the restarted arenas, uint8 [n]."""
        for a, o in enumerate(self.arenas):
            sel = self.mask[a]
            dead = sel & (o.ships()["alive"] == 0)
            finished = dead & (self.dead_once[a] != 0)
            self.dead_once[a][dead] = 1            # a ship already marked stays marked
            death = bool(sel.any()) and bool((finished == sel).all())
            clock = self.max_ticks > 0 and self.time[a] >= self.max_ticks
            self.restarted[a] = 1 if (death or clock) else 0
            self.died[a] = 1 if death else 0
            if not (death or clock):
                self.waiting += int(dead.any())    # a selected ship is dead and the arena waits for the others
                continue
            self.by_death += int(death)
            self.by_clock += int(clock and not death)
            self.arena_episode[a] += 1
            draws = pyoracle.reset_draws(o.cfg, self.seed, self.base + a, int(self.arena_episode[a]))
            self.zero_draws += int((draws == 0).sum())
            g = 0 if self.group is None else int(self.group[a])
            if 0 <= g < self.n_groups:
                self.sums[g, :self.m] += o.ships()["score"]
                self.sums[g, self.m] += 1
                self.sums[g, self.m + 1] += self.time[a]
            o.restart(draws)
            self.time[a] = 0
            self.dead_once[a] = 0
        return self.restarted.copy()

    def step(self, tick):
        """One lock-step of every arena, all ships on the bots' law of the global lock-step `tick`."""
        for a, o in enumerate(self.arenas):
            o.step(o.bot_actions(self.beh, self.seed, self.base + a, tick))
            self.time[a] += 1

    def snapshot(self):
        return dict(ships=[o.ships() for o in self.arenas], lasers=[o.lasers() for o in self.arenas],
                    time=self.time.copy(), arena_episode=self.arena_episode.copy(), dead_once=self.dead_once.copy(),
                    restarted=self.restarted.copy(), sums=self.sums.copy())


_CACHE = {}


def run(seed, m, selected, arena_base=0, group=None, n_groups=1, steps=STEPS, max_ticks=MAX_TICKS, n=N):
    """A scenario, computed once per argument set and never modified: `steps` x (restart_finished, one lock-step on the
    bots' law).  selected: the ship slots selected in every arena, or None = all (the NULL mask).  Returns
    dict(snapshots [steps] (Model.snapshot after each lock-step), heads / dones [steps] (the observation head
    float64 [n][m][8] and done flags AFTER that lock-step's restart_finished, before its step), restarts uint8
    [steps][n], deaths uint8 [steps][n] (those of them that the ships' deaths caused), by_death, by_clock, zero_draws,
    waiting, episodes [n], mask)."""
    key = (seed, m, None if selected is None else tuple(selected), arena_base,
           None if group is None else tuple(int(g) for g in group), n_groups, steps, max_ticks, n)
    if key in _CACHE:
        return _CACHE[key]
    mask = np.ones((n, m), bool) if selected is None else np.zeros((n, m), bool)
    if selected is not None:
        mask[:, list(selected)] = True
    mo = Model(seed, n, m, mask, max_ticks, arena_base, group, n_groups)
    out = dict(snapshots=[], heads=[], dones=[], restarts=np.zeros((steps, n), np.uint8),
               deaths=np.zeros((steps, n), np.uint8))
    for t in range(steps):
        out["restarts"][t] = mo.restart_finished()
        out["deaths"][t] = mo.died
        hd = [o.obs_head() for o in mo.arenas]
        out["heads"].append(np.stack([h for h, _ in hd]))
        out["dones"].append(np.stack([d for _, d in hd]))
        mo.step(t)
        out["snapshots"].append(mo.snapshot())
    out.update(by_death=mo.by_death, by_clock=mo.by_clock, zero_draws=mo.zero_draws, waiting=mo.waiting,
               episodes=mo.arena_episode.copy(), mask=mask)
    out["restarts"].setflags(write=False)
    _CACHE[key] = out
    return out
