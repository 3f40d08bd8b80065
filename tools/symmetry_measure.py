"""How symmetric the game's step is under the eight isometries of the square ("symmetry augmentation";
profiles/r22_augment.txt).  CPU only, on the oracle (oracle/pyoracle.py).

For each of the 7 non-identity elements g: `--episodes` (60) episodes of `--ticks` (8) lock-steps.  Arena A spawns at
seeded draws (clipped to [0, W-1]) with seeded pointings, arena B at the same under g; scripted bots drive A, B receives
A's actions with the pointer under g, both step.  After every lock-step A's ships under g are compared with B's:
position, reward, alive flag.  Two shares per element:
  one-step   over the lock-steps ENTERED from an exactly mirrored state (ships, pointings, alive flags, rewards and every
             laser centre, float64, equal under g): what one transformed transition can get wrong;
  free-run   over all lock-steps of the episodes, differences left to accumulate.
Usage: python tools/symmetry_measure.py [--episodes 60] [--ticks 8]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from oracle import pyoracle

M, SEED = 8, 0x0F160C22
BEHAVIOURS = np.array([1, 2, 3, 1, 4, 5, 1, 2], np.int32)    # random, turret, runner, random, thrust, shoot, random, turret


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def sym(g, x, y, W, H):
    """Element g (include/ofx.h) on positions: arrays of one dtype."""
    if g & 1:
        x, y = y, x
    if g & 2:
        x = (W - 1) - x
    if g & 4:
        y = (H - 1) - y
    return x, y


def mirrored(g, a, b, W, H):
    """Is B's whole state A's under g?  (ships, pointings, flags, rewards, laser centres in listing order)"""
    sa, sb, la, lb = a.ships(), b.ships(), a.lasers(), b.lasers()
    if len(la["x"]) != len(lb["x"]):
        return False
    ok = np.array_equal(np.stack(sym(g, sa["xy"][:, 0], sa["xy"][:, 1], W, H), 1), sb["xy"])
    ok &= np.array_equal(np.stack(sym(g, sa["pt"][:, 0], sa["pt"][:, 1], W, H), 1), sb["pt"])
    ok &= np.array_equal(sa["alive"], sb["alive"]) and np.array_equal(sa["reward"], sb["reward"])
    lx, ly = sym(g, la["x"], la["y"], W, H)
    return bool(ok and np.array_equal(lx, lb["x"]) and np.array_equal(ly, lb["y"]) and
                np.array_equal(la["destroyed"], lb["destroyed"]))


def measure(g, episodes, ticks):
    cfg = pyoracle.default_cfg(M)
    W, H = cfg.width, cfg.height
    stats = {k: dict(n=0, pos=0, reward=0, alive=0, any=0, dmax=0) for k in ("one-step", "free-run")}
    for ep in range(episodes):
        a, b = pyoracle.Arena(n_ships=M), pyoracle.Arena(n_ships=M)
        draws = np.minimum(pyoracle.reset_draws(cfg, SEED, ep, 0), W - 1)
        point = np.random.RandomState(ep).randint(0, W, (M, 2))
        a.spawn(draws)
        b.spawn(np.stack(sym(g, draws[:, 0], draws[:, 1], W, H), 1))
        for i in range(M):
            a.set_ship(i, draws[i, 0], draws[i, 1], point[i, 0], point[i, 1])
            b.set_ship(i, *sym(g, draws[i, 0], draws[i, 1], W, H), *sym(g, point[i, 0], point[i, 1], W, H))
        for t in range(ticks):
            clean = mirrored(g, a, b, W, H)
            act = a.bot_actions(BEHAVIOURS, SEED, ep, t)
            act_b = act.copy()
            act_b[:, 3], act_b[:, 4] = sym(g, act[:, 3], act[:, 4], W, H)
            a.step(act)
            b.step(act_b)
            sa, sb = a.ships(), b.ships()
            want = np.stack(sym(g, sa["xy"][:, 0], sa["xy"][:, 1], W, H), 1)
            d = np.abs(want.astype(np.int64) - sb["xy"]).max(1)
            pos, rew, alive = d != 0, sa["reward"] != sb["reward"], sa["alive"] != sb["alive"]
            for key in (("one-step",) if clean else ()) + ("free-run",):
                s = stats[key]
                s["n"] += M
                s["pos"] += int(pos.sum())
                s["reward"] += int(rew.sum())
                s["alive"] += int(alive.sum())
                s["any"] += int((pos | rew | alive).sum())
                s["dmax"] = max(s["dmax"], int(d.max()))
    return stats


if __name__ == "__main__":
    episodes, ticks = _arg("--episodes", 60), _arg("--ticks", 8)
    print("element   mode      ship-steps   position   reward     alive      any        largest |dx|,|dy|")
    for g in range(1, 8):
        for key, s in measure(g, episodes, ticks).items():
            n = max(s["n"], 1)
            print("g = %d     %-9s %-12d %-10s %-10s %-10s %-10s %d" % (
                g, key, s["n"], *("%.3f %%" % (100.0 * s[k] / n) for k in ("pos", "reward", "alive", "any")), s["dmax"]))
