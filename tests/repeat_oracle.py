"""Action repeat (ofx_step_repeat, include/ofx.h) restated on the CPU oracle: a span is K x (the bots' law of lock-step
tick0 + j, the held ships' rows overwritten by their held action, one oracle step).  The GPU tests compare against this
model; tests/test_action_repeat.py asserts, on the model alone, that the scenario below exercises what it must."""
import numpy as np

from oracle import pyoracle

N, M, W, H = 5, 8, 400, 400                       # 5 arenas: not a multiple of the 4 arenas of a block
REWARDS = dict(reward_death=-5, reward_kill=7)
BEHAVIOURS = ["shoot", "turret", "runner", "random", "turret", "thrust", "random", "turret"]
HELD = (0, 3)
K, SPANS, SEED = 4, 12, 12345
ACTION_SEED = 11                                  # numpy.random.RandomState of the held actions: with it the scenario
                                                  # meets all four conditions test_action_repeat.py asserts (12345 misses one)
BOT = {None: 0, "idle": 0, "random": 1, "turret": 2, "runner": 3, "thrust": 4, "shoot": 5}   # OFX_BOT_* (include/ofx.h)


def span_oracle(arena, beh, seed, g, tick0, K, held):
    """Advance `arena` (a pyoracle.Arena, global arena id g) by one span of K lock-steps.  beh: int32 [M] OFX_BOT_*;
    held: {ship: (valid, shoot, thrust, px, py)}, played on every lock-step (the oracle's step applies `valid and alive`
    itself, as ofx_step does).  Returns the rewards earned per lock-step, int64 [K][M]."""
    out = np.zeros((K, arena.M), np.int64)
    for j in range(K):
        act = arena.bot_actions(beh, seed, g, tick0 + j)
        for i, a in held.items():
            act[i] = a
        arena.step(act)
        out[j] = arena.ships()["reward"]
    return out


def spawn(seed, n=N, m=M, **cfg):
    arenas = []
    for g in range(n):
        o = pyoracle.Arena(cfg=pyoracle.default_cfg(m, **dict(REWARDS, **cfg)))
        o.spawn(pyoracle.reset_draws(o.cfg, seed, g, 0))
        arenas.append(o)
    return arenas


def draw_held(rs, alive, held, w=W, h=H):
    """One decision of the held ships of every arena: valid = alive now, exactly one of shoot / thrust, a uniform
    pointer.  alive: uint8 [n][m].  Returns int32 [n][m][5] = valid, shoot, thrust, px, py (zero rows elsewhere)."""
    n, m = alive.shape
    act = np.zeros((n, m, 5), np.int32)
    for g in range(n):
        for i in held:
            shoot = int(rs.randint(0, 2))
            act[g, i] = (int(alive[g, i]), shoot, 1 - shoot, int(rs.randint(0, w)), int(rs.randint(0, h)))
    return act


_CACHE = {}


def scenario(m=M, behaviours=BEHAVIOURS, held=HELD, k=K, spans=SPANS, seed=SEED, restart_after=None, action_seed=ACTION_SEED):
    """The scripted run shared by the CPU and the GPU tests, computed once per argument set and never modified:
    `spans` spans of k lock-steps from spawn, the held actions drawn per span from numpy.random.RandomState(action_seed);
    restart_after = s restarts every arena (episode 1) between span s and span s + 1.
    Returns dict(actions [spans][N][m][5], alive0 [spans][N][m] (alive at the decision), rewards [spans][k][N][m],
    alive_before [spans][k][N][m] (alive when the lock-step began), ships / lasers: the oracles' final state)."""
    key = (m, tuple(behaviours), tuple(held), k, spans, seed, restart_after, action_seed)
    if key in _CACHE:
        return _CACHE[key]
    beh = np.array([BOT[b] for b in behaviours], np.int32)
    arenas = spawn(seed, N, m)
    rs = np.random.RandomState(action_seed)
    out = dict(actions=np.zeros((spans, N, m, 5), np.int32), alive0=np.zeros((spans, N, m), np.uint8),
               rewards=np.zeros((spans, k, N, m), np.int64), alive_before=np.zeros((spans, k, N, m), np.uint8))
    for s in range(spans):
        alive = np.stack([o.ships()["alive"] for o in arenas])
        out["alive0"][s] = alive
        out["actions"][s] = draw_held(rs, alive, held)
        for g, o in enumerate(arenas):
            for j in range(k):                     # one lock-step at a time, to see who was alive when it began
                out["alive_before"][s, j, g] = o.ships()["alive"]
                out["rewards"][s, j, g] = span_oracle(o, beh, seed, g, s * k + j, 1,
                                                      {i: out["actions"][s, g, i] for i in held})[0]
        if restart_after is not None and s == restart_after:
            for g, o in enumerate(arenas):
                o.restart(pyoracle.reset_draws(o.cfg, seed, g, 1))
    out["ships"] = [o.ships() for o in arenas]
    out["lasers"] = [o.lasers() for o in arenas]
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CACHE[key] = out
    return out
