"""What the symmetry augmentation costs (profiles/r22_augment.txt).

kernel   ofx_replay_augment alone on `--rows` gathered rows (random disc maps built on the host, the first 256 repeated),
         between the handle's timer events: `--calls` (20) calls per timing, 3 warm-up calls, 5 timings per mask; masks 0x55
         (flips), 0xFF (d4), 0xAA (transposing elements only) and 0x54 (mirrors and half turn only, no identity).  Next
         to each time stand the bytes the call must move (every transformed observation read and written once: 2 x 80 KB
         per row less the rows that drew the identity) and the rate that makes.
replay   DeviceTrainer.replay per call at `--arenas` (4096) arenas x 8 ships, one policy ship, memory 64, frames 96,
         fit_batch 256: 40 training lock-steps fill the memories, 5 warm-up replays, then `--repeats` (5) blocks of 20
         replays, ms per replay each.  `--augment NAME` (flips, d4) turns the option on; without it the file uses only what
         the trainer had before the option, so it also times a copy of the parent commit (`--tree NAME` labels the line).
Usage: python tools/augment_time.py [kernel] [replay] [--rows 256] [--arenas 4096] [--calls 20] [--repeats 5]
                                    [--augment NAME] [--tree NAME]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from ofighters_amd import ArenaBatch, DeviceBuffer
from ofighters_amd.agents.policy_weights import synthetic
from ofighters_amd.lib.epsilon import Epsilon_decay
from ofighters_amd.rollout import TrainingRollout
from ofighters_amd.trainer import DeviceTrainer

M, SEED, SIDE = 8, 0x0F160B22, 400


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def _maps(n):
    """uint32 [n][2][5000]: six ship discs of radius 8 and six laser discs of radius 3 per observation"""
    rs = np.random.RandomState(22)
    yy, xx = np.ogrid[:SIDE, :SIDE]
    u = min(n, 256)
    maps = np.zeros((u, 2, SIDE, SIDE), bool)
    for k in range(u):
        for plane, r in ((0, 8), (1, 3)):
            for cy, cx in rs.randint(0, SIDE, (6, 2)):
                maps[k, plane] |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    bits = np.packbits(maps.reshape(u, 2, -1), axis=-1, bitorder="little").view(np.uint32)
    return np.ascontiguousarray(np.tile(bits, ((n + u - 1) // u, 1, 1))[:n])


def kernel():
    n, calls = _arg("--rows", 256), _arg("--calls", 20)
    b = ArenaBatch(1, 1)
    bits = _maps(n)
    d_prev, d_next = DeviceBuffer(bits.nbytes).upload(bits), DeviceBuffer(bits.nbytes).upload(bits[::-1])
    rows = np.zeros(n, b.TRANSITION_DTYPE)
    rows["head_prev"][:, 4:6] = rows["head_next"][:, 4:6] = SIDE
    d_rows, d_op = DeviceBuffer(rows.nbytes).upload(rows), DeviceBuffer(n)
    out = {"what": "kernel", "rows": n, "calls": calls}
    for mask in (0x55, 0xFF, 0xAA, 0x54):
        ms = []
        for rep in range(6):                                 # the first timing is the warm-up
            b.timer_start()
            for k in range(3 if rep == 0 else calls):
                b.replay_augment_into(SEED, rep * calls + k, 0, n, mask, d_rows, d_prev, d_next, d_op)
            t = b.timer_stop()
            if rep:
                ms.append(t / calls)
        moved = int((d_op.download(np.uint8, (n,)) != 0).sum())   # of the last call; every draw's share is about the same
        gb = moved * 2 * 2 * bits[0].nbytes / 1e9
        out["0x%02X" % mask] = {"ms_per_call": [round(x, 4) for x in ms], "mean_ms": round(float(np.mean(ms)), 4),
                                "rows_transformed": moved, "GB_moved": round(gb, 4),
                                "TB_per_s": round(gb / float(np.mean(ms)), 3)}
    b.close()
    return out


def replay():
    repeats = _arg("--repeats", 5)
    opt = {}
    if "--augment" in sys.argv:
        opt["augment"] = _arg("--augment", "d4")
    b = ArenaBatch(_arg("--arenas", 4096), M)
    eps = Epsilon_decay()
    eps.set(0.1)
    tr = DeviceTrainer(b, synthetic(), epsilon=eps, batch_size=8, memory_size=64, frames=96, fit_batch=256, **opt)
    roll = TrainingRollout(b, tr, ["random"] * M, SEED, policy_ships=(0,), episode_ticks=b.cfg.episode_ticks)
    roll.run(40)
    for _ in range(5):
        tr.replay()
    b.sync()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(20):
            tr.replay()
        b.sync()
        ms.append((time.perf_counter() - t0) / 20 * 1e3)
    out = {"what": "replay", "tree": _arg("--tree", "this commit"), "options": opt, "arenas": b.N, "fit_batch": 256,
           "ms_per_replay": [round(x, 4) for x in ms], "min_ms": round(min(ms), 4), "mean_ms": round(float(np.mean(ms)), 4),
           "loss": [float(x) for x in tr.losses[-1]]}
    b.close()
    return out


if __name__ == "__main__":
    what = [x for x in sys.argv[1:] if x in ("kernel", "replay")] or ["kernel", "replay"]
    for name, fn in (("kernel", kernel), ("replay", replay)):
        if name in what:
            print(json.dumps(fn()), flush=True)
