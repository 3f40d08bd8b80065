"""The member queue of the evolution strategy (ofx_es_requeue, ofx_restart_arenas; include/ofx.h) restated on the CPU:
the requeue law in numpy, line for line as the header states it, ofx_restart_arenas on top of
tests/autoreset_oracle.Model, a generation driven by that model, and the seeded cases the GPU test of the law uploads.
A helper module (not collected); tests/test_es_queue.py asserts, on this module alone, that the scenarios exercise what
they must."""
import numpy as np

from oracle import pyoracle
from tests import autoreset_oracle as ao
from tests import repeat_oracle as ro


def requeue(restarted, member_of, queue_mask, last_score, P, total, queue, sum, count, bank):
    """The law, in place on member_of int32 [N][M], queue int64 [2], sum int64 [P + 1] and count int32 [P + 1].
    Returns the tickets handed out as a list of (a, i, ticket), and the (a, i) that asked and got -1."""
    N, M = member_of.shape
    handed, refused = [], []
    next, completed = int(queue[0]), int(queue[1])
    for a in range(N):
        if restarted[a] == 0:
            continue
        for i in range(M):
            m = int(member_of[a, i])
            if bank != 0 and 0 <= m <= P:
                sum[m] += int(last_score[a, i])
                count[m] += 1
                if m < P:
                    completed += 1
            if queue_mask[a, i] != 0:
                if next < total:
                    member_of[a, i] = next % P
                    handed.append((a, i, next))
                    next += 1
                else:
                    member_of[a, i] = -1
                    refused.append((a, i))
    queue[0], queue[1] = next, completed
    return handed, refused


class Model(ao.Model):
    """autoreset_oracle.Model on arenas of width x height (None: the default map), with ofx_restart_arenas."""

    def __init__(self, seed, n, m, mask, max_ticks, width=None, height=None, **kw):
        super().__init__(seed, n, m, mask, max_ticks, **kw)
        if width is not None:
            self.arenas = []
            for a in range(n):
                o = pyoracle.Arena(cfg=pyoracle.default_cfg(m, width=width, height=height, **ro.REWARDS))
                o.spawn(pyoracle.reset_draws(o.cfg, seed, self.base + a, 0))
                self.arenas.append(o)

    def restart_arenas(self, arena_mask=None):
        """One call of ofx_restart_arenas; arena_mask: [n] or None = all.  Returns the restarted arenas, uint8 [n]."""
        for a, o in enumerate(self.arenas):
            go = arena_mask is None or arena_mask[a] != 0
            self.restarted[a] = 1 if go else 0
            if not go:
                continue
            self.arena_episode[a] += 1
            o.restart(pyoracle.reset_draws(o.cfg, self.seed, self.base + a, int(self.arena_episode[a])))
            self.time[a] = 0
            self.dead_once[a] = 0
        return self.restarted.copy()

    def last_score(self):
        return np.stack([o.ships()["last_score"] for o in self.arenas]).astype(np.int32)


GENERATION = dict(seed=777, n=5, m=8, selected=(0, 3), max_ticks=40, P=16, E=2)
_CACHE = {}


def generation(seed, n, m, selected, max_ticks, P, E, limit=4000):
    """One generation of the queue on the autoreset model, every ship on the bots' law: begin (all ships of `selected`
    idle, restart_arenas on all arenas, requeue without banking), then (restart_finished, requeue, one lock-step) until
    completed == total.  Computed once per argument set and never modified.  Returns dict(calls: per requeue call
    (handed, refused, completed after it, restarted), count, sum, member_of, queue, by_death, by_clock, ticks)."""
    key = (seed, n, m, tuple(selected), max_ticks, P, E)
    if key in _CACHE:
        return _CACHE[key]
    mask = np.zeros((n, m), bool)
    mask[:, list(selected)] = True
    mo = Model(seed, n, m, mask, max_ticks)
    total = E * P
    member_of = np.full((n, m), -1, np.int32)
    queue, sum, count = np.zeros(2, np.int64), np.zeros(P + 1, np.int64), np.zeros(P + 1, np.int32)
    calls = []

    def call(restarted, bank):
        handed, refused = requeue(restarted, member_of, mask, mo.last_score(), P, total, queue, sum, count, bank)
        calls.append((handed, refused, int(queue[1]), restarted.copy()))

    call(mo.restart_arenas(), 0)
    tick = 0
    while queue[1] < total:
        assert tick < limit, "the generation does not end"
        call(mo.restart_finished(), 1)
        if queue[1] == total:
            break
        mo.step(tick)
        tick += 1
    out = dict(calls=calls, count=count, sum=sum, member_of=member_of, queue=queue, by_death=mo.by_death,
               by_clock=mo.by_clock, ticks=tick, total=total)
    _CACHE[key] = out
    return out


# ---------------------------------------------------------------- the cases of the law the GPU test uploads
LAW_SHAPES = [(n, m) for n in (1, 5, 257, 1030) for m in (3, 13)]
LAW_P = 10


def law_inputs(n, m, P=LAW_P):
    """(arena_mask uint8 [n], member_of int32 [n][m], queue_mask uint8 [n][m]) of the shape, from a seed of its own:
    member_of holds -1, P, in-range values with duplicates, and the out-of-range -2 and P + 1."""
    rs = np.random.RandomState(1000 * n + m)
    arena_mask = (rs.rand(n) < 0.6).astype(np.uint8)
    arena_mask[0] = 1                                            # the one arena of n = 1 restarts
    member_of = rs.choice(np.array([-2, -1, -1, P, P + 1] + list(range(P)) + [3, 3, 3], np.int32), (n, m))
    member_of = member_of.astype(np.int32)
    queue_mask = (rs.rand(n, m) < 0.5).astype(np.uint8)
    return arena_mask, member_of, queue_mask


def law_queues(arena_mask, queue_mask):
    """The (next, completed, total) states a shape is called with: a queue that serves everybody, one that runs out a
    few tickets short of what is asked, and the empty one (total = 0)."""
    asks = int(queue_mask[arena_mask != 0].sum())
    short = max(asks - 3, 0) if asks > 1 else 0
    return [(7, 5, 7 + asks + 100), (41, 2, 41 + short), (0, 0, 0)]
