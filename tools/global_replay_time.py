"""Global minibatch sampling against the per-arena samplers at the training tick's size (profiles/r10_global_replay.txt):
`--arenas` (4096) arenas x 8 ships, one policy ship, memory_size 400, the memory filled by `--steps` (2500) training
lock-steps of the mode under test (TrainingRollout, ["random"] * 8, episode_ticks 200, batch_size 8, fit_batch 256).
Modes: per_arena (the default trainer), global_uniform, global_per (global_sampling + prioritized).  Per mode, `--reps`
times each of
  replay   wall time of one DeviceTrainer.replay at 256 rows, median of 20 after 3 warm-up calls (ends in the fit's
           synchronise)
  front    the sample + gather part of replay() alone - the trainer's own calls up to the gather, host round trips
           included - between two HIP events on the handle's stream, median of 20 after 3 warm-up calls
Usage: python tools/global_replay_time.py [--arenas 4096] [--steps 2500] [--reps 3] [--modes per_arena,global_uniform,global_per]
                                          [--packed] [--package DIR] [--stats]
--package DIR imports ofighters_amd from DIR instead of this tree; with --modes per_arena nothing this feature added is
named, so it runs on a checkout from before it: two builds on one card in one session.
--stats instead fills a prioritized memory, spreads its priorities by hand over six decades (no fit in between, so they
stay put) and records over `--draws` (40) replays' worth of sampling: the share of the memory's top-1 % masses among the
rows the per-arena prioritized window would fit and among the rows the global prioritized sampler draws, and the fraction
of the latter that come from arenas outside the per-arena window of the same draw."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


PKG = os.path.abspath(_arg("--package", ROOT))
sys.path.insert(0, PKG)
import numpy as np

from ofighters_amd import ArenaBatch, DeviceBuffer
from ofighters_amd.agents.policy_weights import synthetic
from ofighters_amd.lib.epsilon import Epsilon_decay
from ofighters_amd.rollout import TrainingRollout
from ofighters_amd.trainer import DeviceTrainer

M, CAP, SEED, FIT = 8, 400, 0x0F160061, 256
ARENAS, STEPS, REPS = _arg("--arenas", 4096), _arg("--steps", 2500), _arg("--reps", 3)
MODES = {"per_arena": {}, "global_uniform": dict(global_sampling=True),
         "global_per": dict(global_sampling=True, prioritized=True), "per_arena_per": dict(prioritized=True)}


def build(mode):
    b = ArenaBatch(ARENAS, M)
    eps = Epsilon_decay()
    eps.set(0.1)
    kw = dict(MODES[mode])                                   # nothing new is named on the default path (--package)
    if "--packed" in sys.argv:
        kw["packed_memory"] = True
    tr = DeviceTrainer(b, synthetic(), epsilon=eps, batch_size=8, memory_size=CAP, fit_batch=FIT, seed=SEED, **kw)
    roll = TrainingRollout(b, tr, ["random"] * M, SEED, policy_ships=(0,), episode_ticks=200)
    return b, tr, roll


def run(b, roll, n):
    t0 = time.perf_counter()
    roll.run(n)
    b.sync()
    return time.perf_counter() - t0


def window(tr, prioritized):
    """The per-arena replay()'s own calls up to the gather (trainer.py): -> (slot, n_s, bs, start, n) or None."""
    b, bs = tr.batch, int(tr.batch_size)
    cnt, _ = b.replay_count()
    if int(cnt.max()) == 0:
        return None
    if prioritized:
        slot, n_s, _ = b.replay_sample_prioritized(tr.seed, tr.draws, bs, tr.beta(), tr._scratch("slot", 4 * b.N * bs),
                                                   tr._scratch("n_s", 4 * b.N), tr._scratch("is_w", 4 * b.N * bs))
    else:
        slot, n_s = b.replay_sample(tr.seed, tr.draws, bs, tr._scratch("slot", 4 * b.N * bs), tr._scratch("n_s", 4 * b.N))
    tr.draws += 1
    b.sync()
    n_valid = int(n_s.download(np.int32, (b.N,)).sum())
    n = min(n_valid, int(tr.fit_batch))
    return slot, n_s, bs, ((tr.draws - 1) * n) % (n_valid - n + 1), n


def front(tr):
    """Sample + gather as replay() does them, without targets and fit; the draw counter moves as in replay()."""
    b = tr.batch
    words = b.W * b.H // 32
    nb = int(tr.fit_batch)
    rows = tr._scratch("rows", nb * b.TRANSITION_DTYPE.itemsize)
    bp, bn = tr._scratch("bits_prev", 8 * nb * words), tr._scratch("bits_next", 8 * nb * words)
    if getattr(tr, "global_sampling", False):
        arena, slot, _, n, _ = b.replay_sample_global(tr.seed, tr.draws, nb, tr.prioritized, tr.beta() if tr.prioritized else 0.0,
                                                      tr._scratch("g_arena", 4 * nb), tr._scratch("g_slot", 4 * nb),
                                                      tr._scratch("row_w", 4 * nb) if tr.prioritized else None)
        tr.draws += 1
        b.replay_gather_list_into(arena, slot, n, rows, bp, bn)
    else:
        slot, n_s, bs, start, n = window(tr, tr.prioritized)
        b.replay_gather_valid_into(slot, n_s, bs, start, n, rows, bp, bn)


def measure(mode):
    b, tr, roll = build(mode)
    out = {"mode": mode, "arenas": ARENAS, "packed": "--packed" in sys.argv, "fill_steps": STEPS, "fill_s": run(b, roll, STEPS),
           "fits": tr.fit_steps, "rows": int(b.replay_count()[0].sum()), "replay_ms": [], "front_ms": []}
    for _ in range(REPS):
        ts = []
        for _ in range(23):
            t0 = time.perf_counter()
            tr.replay()
            ts.append((time.perf_counter() - t0) * 1e3)
        out["replay_ms"].append(float(np.median(ts[3:])))
        ms = []
        for _ in range(23):
            b.timer_start()
            front(tr)
            ms.append(b.timer_stop())
        out["front_ms"].append(float(np.median(ms[3:])))
    out["losses_finite"] = bool(np.isfinite(np.array(tr.losses)).all())
    b.close()
    return out


def stats():
    draws = _arg("--draws", 40)
    b, tr, roll = build("per_arena_per")
    run(b, roll, STEPS)
    N = b.N
    # hand-spread priorities: every eligible row once through the list write-back, |td| = 10^U(-3, 3)
    R = int(b.replay_count()[0].sum())
    arena, slot, _, n, elig = b.replay_sample_global(SEED, 0, R)
    rows = DeviceBuffer(n * b.TRANSITION_DTYPE.itemsize)
    b.replay_gather_list_into(arena, slot, n, rows, None, None)
    td = np.zeros((n, 2), np.float32)
    td[:, 0] = 10.0 ** np.random.RandomState(1).uniform(-3, 3, n)
    td_d = DeviceBuffer(td.nbytes).upload(td)                           # held until the sync: the write-back is asynchronous
    b.replay_update_priorities_list(arena, slot, n, rows.ptr, td_d.ptr)
    b.sync()
    mass = [b.replay_priorities(a) for a in range(N)]
    top = np.sort(np.concatenate(mass))[-max(1, elig // 100)]            # the top-1 % threshold
    out = {"arenas": N, "fill_steps": STEPS, "rows": R, "eligible": int(elig), "top1pct_mass": float(top), "draws": draws,
           "fitted_window": 0, "fitted_global": 0, "top_window": 0, "top_global": 0, "outside_window": 0}
    for d in range(draws):
        tr.draws = d + 1
        slot_d, n_s, bs, start, n = window(tr, True)
        sl, ns = slot_d.download(np.int32, (N, bs)), n_s.download(np.int32, (N,))
        off = np.concatenate([[0], np.cumsum(ns)])
        win_arenas = set()
        for e in range(start, start + n):                                # packed (arena, j) order
            a = int(np.searchsorted(off, e, side="right") - 1)
            win_arenas.add(a)
            out["top_window"] += int(mass[a][sl[a, e - off[a]]] >= top)
        out["fitted_window"] += n
        ga, gs, _, gn, _ = b.replay_sample_global(SEED, d + 1, FIT, True, tr.beta())
        b.sync()
        ga, gs = ga.download(np.int32, (FIT,))[:gn], gs.download(np.int32, (FIT,))[:gn]
        out["fitted_global"] += int(gn)
        out["top_global"] += int(sum(mass[a][s] >= top for a, s in zip(ga, gs)))
        out["outside_window"] += int(sum(a not in win_arenas for a in ga))
    out["top_share_window"] = out["top_window"] / out["fitted_window"]
    out["top_share_global"] = out["top_global"] / out["fitted_global"]
    out["outside_window_frac"] = out["outside_window"] / out["fitted_global"]
    b.close()
    return out


if __name__ == "__main__":
    print(json.dumps({"package": os.path.relpath(PKG, ROOT), "argv": sys.argv[1:]}))
    if "--stats" in sys.argv:
        print(json.dumps(stats()), flush=True)
    else:
        for mode in _arg("--modes", "per_arena,global_uniform,global_per").split(","):
            print(json.dumps(measure(mode)), flush=True)
