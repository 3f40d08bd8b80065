"""Per-arena episodes at the training size (profiles/r18_auto_reset.txt): `--arenas` (4096) arenas x 8 ships, one policy
ship, TrainingRollout + DeviceTrainer (memory 64, frames 96, fit_batch 256, replays on the reference's schedule).

tick     `--modes off,on` (default): one rollout per mode in ONE process, each on its own handle and trainer, 32 warm-up
         lock-steps (the collecting phase is the first 20), then `--blocks` (6) timed blocks of `--block` (100)
         lock-steps per mode, ALTERNATING between the modes (a host clock around work that ends in a synchronise), then
         one untimed pass of `--alive-steps` (200, one global episode) lock-steps per mode that downloads the policy
         ships' alive flags at every forward.  Per mode: ms per lock-step, rows appended per lock-step
         (replay_count's `appended`) and fits over the timed lock-steps, the share of policy ships alive at the forward,
         and with auto_reset the mean episode length from length_log / score_log.  With `--modes off` it passes nothing
         the rollout did not have before the option, so the same file times a copy of the parent commit: `--root PATH`
         imports the package from that tree and `--tree NAME` labels the line.
kernel   ofx_restart_finished alone, from HIP events on the handle's stream (ofx_event_record / ofx_event_elapsed), one
         event pair per call, `--calls` (200) calls with one lock-step of the bots between two of them, ship 0 selected,
         max_ticks 200, sums and a `seen` array given: without a replay memory (the one kernel) and with one (the kernel
         and the reset of the restarted arenas' agents); us per call and the restarts it made.
Each mode prints one JSON line and, with `--out FILE`, appends it to that file.
Usage: python tools/auto_reset_time.py tick|kernel [--arenas 4096] [--modes off,on] [--block 100] [--blocks 6]
                                       [--alive-steps 200] [--calls 200] [--root PATH] [--tree NAME] [--out FILE]

One GPU step per process, each under its own time limit, chained so that a failure ends the chain:
    timeout -k 10 300 python tools/auto_reset_time.py kernel --out profiles/r18_auto_reset.txt \\
    && timeout -k 10 600 python tools/auto_reset_time.py tick --out profiles/r18_auto_reset.txt"""
import json
import os
import sys
import time


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


ROOT = os.path.abspath(_arg("--root", os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)
import numpy as np

from ofighters_amd import ArenaBatch, DeviceBuffer, _native as nat
from ofighters_amd.agents.policy_weights import synthetic
from ofighters_amd.lib.epsilon import Epsilon_decay
from ofighters_amd.rollout import TrainingRollout
from ofighters_amd.trainer import DeviceTrainer

M, SEED = 8, 0x0F160111
ARENAS = _arg("--arenas", 4096)


class _Run:
    def __init__(self, mode):
        self.mode = mode
        self.b = ArenaBatch(ARENAS, M)
        eps = Epsilon_decay()
        eps.set(0.1)
        self.tr = DeviceTrainer(self.b, synthetic(), epsilon=eps, batch_size=8, memory_size=64, frames=96, fit_batch=256)
        kw = dict(auto_reset=True) if mode == "on" else {}
        self.roll = TrainingRollout(self.b, self.tr, ["random"] * M, SEED, policy_ships=(0,),
                                    episode_ticks=self.b.cfg.episode_ticks, **kw)
        self.ms, self.rows, self.fits, self.steps = [], 0, 0, 0

    def appended(self):
        return int(self.b.replay_count()[1].sum())

    def block(self, n):
        r0, f0 = self.appended(), self.tr.fit_steps
        self.b.sync()
        t0 = time.perf_counter()
        self.roll.run(n)
        self.b.sync()
        self.ms.append((time.perf_counter() - t0) * 1e3 / n)
        self.rows += self.appended() - r0
        self.fits += self.tr.fit_steps - f0
        self.steps += n

    def alive_share(self, n):
        """The share of policy ships alive when _play runs (after that lock-step's restarts), over n lock-steps."""
        seen, play = [0], self.roll.policy

        def sampled(e):
            seen[0] += int(e.get(nat.F_SHIP_ALIVE)[:, 0].sum())
            return play(e)
        self.roll.policy = sampled
        self.roll.run(n)
        self.roll.policy = play
        return seen[0] / float(n * ARENAS)

    def result(self, alive):
        out = {"mode": self.mode, "ms_per_lock_step": [round(x, 4) for x in self.ms],
               "mean_ms_per_lock_step": round(float(np.mean(self.ms)), 4), "timed_lock_steps": self.steps,
               "rows_per_lock_step": round(self.rows / float(self.steps), 2), "fits": self.fits,
               "alive_share": round(alive, 4), "end_tick": int(self.roll.tick), "periods": len(self.roll.score_log)}
        if self.mode == "on":
            eps = sum(int(x[M]) for x in self.roll.score_log)
            out["episodes_finished"] = eps
            out["mean_episode_length"] = round(sum(int(x.sum()) for x in self.roll.length_log) / float(max(eps, 1)), 2)
        return out


def tick():
    modes = _arg("--modes", "off,on").split(",")
    block, blocks, alive_steps = _arg("--block", 100), _arg("--blocks", 6), _arg("--alive-steps", 200)
    runs = [_Run(m) for m in modes]
    for r in runs:
        r.roll.run(32)
    for _ in range(blocks):
        for r in runs:
            r.block(block)
    alive = [r.alive_share(alive_steps) for r in runs]
    out = {"what": "tick", "tree": _arg("--tree", "this commit"), "arenas": ARENAS, "block": block, "blocks": blocks,
           "alive_steps": alive_steps, "runs": [r.result(a) for r, a in zip(runs, alive)]}
    for r in runs:
        r.b.close()
    return out


def kernel():
    calls = _arg("--calls", 200)
    beh = ["random"] * M
    mk = np.zeros((ARENAS, M), np.uint8)
    mk[:, 0] = 1
    out = {"what": "kernel", "arenas": ARENAS, "ships": M, "calls": calls, "max_ticks": 200, "variants": {}}
    for name in ("no replay memory", "with a replay memory"):
        b = ArenaBatch(ARENAS, M)
        if name.startswith("with"):
            b.replay_create(64, 96)
        b.spawn_random(SEED)
        b.rollout(beh, SEED, 0, 40)                              # lasers in flight, some ships destroyed
        mask = DeviceBuffer(mk.nbytes).upload(mk)
        seen = DeviceBuffer(mk.nbytes).upload(np.zeros_like(mk))
        sums = DeviceBuffer(8 * (M + 2)).upload(np.zeros(M + 2, np.int64))
        for j in range(10):                                      # warm-up (the first call allocates)
            b.restart_finished(SEED, mask.ptr, 200, seen, None, 1, sums)
            b.rollout(beh, SEED, 40 + j, 1)
        b.sync()
        sums.upload(np.zeros(M + 2, np.int64))
        for j in range(calls):
            b.event_record(2 * j)
            b.restart_finished(SEED, mask.ptr, 200, seen, None, 1, sums)
            b.event_record(2 * j + 1)
            b.rollout(beh, SEED, 50 + j, 1)
        b.sync()
        us = np.array([b.event_elapsed(2 * j, 2 * j + 1) for j in range(calls)]) * 1e3
        out["variants"][name] = {"mean_us": round(float(us.mean()), 2), "median_us": round(float(np.median(us)), 2),
                                 "min_us": round(float(us.min()), 2), "max_us": round(float(us.max()), 2),
                                 "restarts": int(sums.download(np.int64, (M + 2,))[M])}
        b.close()
    return out


if __name__ == "__main__":
    what = [x for x in sys.argv[1:] if x in ("tick", "kernel")]
    if len(what) != 1:
        raise SystemExit(__doc__)
    line = json.dumps(tick() if what[0] == "tick" else kernel())
    print(line, flush=True)
    if "--out" in sys.argv:
        with open(_arg("--out", ""), "a") as f:
            f.write(line + "\n")
