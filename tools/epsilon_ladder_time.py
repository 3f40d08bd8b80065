"""The exploration ladder's cost at the training size (profiles/r14_epsilon_ladder.txt): `--arenas` (4096) arenas x 8 ships.

kernels  One handle, weights pinned, every ship a policy ship for the explore, one per arena for the act.  Each call is
         timed with ofx_timer_* around `--block` (50) calls in a row (one synchronisation per block), in alternating
         blocks without (A) and with (B) an Ape-X ladder (alpha 7, 64 greedy arenas), `--blocks` (10) blocks each after
         two warm-up blocks.  The ladder is set and removed between blocks (a synchronising set-up call, not timed).
           explore  ofx_policy_explore at epsilon 0.5
           act      ofx_policy_act at epsilon 0.5 (the forward dominates)
         Then ofx_episode_scores_grouped with 9 groups (8 bands + the evaluation group) and, for scale,
         ofx_episode_scores, the same way.
tick     The training tick of bench.py's secondary line (TrainingRollout, one policy ship per arena, memory 64, frames
         96, fit_batch 256, replays on the reference's schedule): 30 warm-up lock-steps, then `--repeats` (5) timed runs
         of 120 lock-steps, ms per lock-step each.  Uses only what the rollout had before the options, so the same file
         times a copy of the parent commit (`--tree NAME` labels the line); `--ladder` turns epsilon_ladder=7,
         eval_arenas=64 on.
Usage: python tools/epsilon_ladder_time.py [kernels] [tick] [--arenas 4096] [--block 50] [--blocks 10] [--repeats 5] [--ladder]
                                           [--tree NAME]"""
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

M, SEED, EVAL = 8, 0x0F160081, 64


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


ARENAS = _arg("--arenas", 4096)


def _stats(ms):
    a = np.array(ms)
    return {"blocks_us": [round(1e3 * float(x), 2) for x in a], "mean_us": round(1e3 * float(a.mean()), 2),
            "min_us": round(1e3 * float(a.min()), 2), "spread_us": round(1e3 * float(a.max() - a.min()), 2)}


def kernels():
    from ofighters_amd.exploration import apex_exponents, score_groups
    block, blocks = _arg("--block", 50), _arg("--blocks", 10)
    b = ArenaBatch(ARENAS, M)
    b.spawn_random(SEED)
    w = synthetic()
    dw = DeviceBuffer(w.nbytes).upload(w)
    mk = np.zeros((ARENAS, M), np.uint8)
    mk[:, 0] = 1
    one_buf = DeviceBuffer(mk.nbytes).upload(mk)             # kept: the pointer alone would outlive its buffer
    one = one_buf.ptr
    b.policy_pin_weights(dw.ptr)
    for t in range(3):                                       # a few lock-steps: the maps are not the empty start
        b.bot_actions(["random"] * M, SEED, tick=t)
        b.step()
    b.rasterise()
    expo = apex_exponents(ARENAS, 7.0, 0, ARENAS, EVAL)
    tick = [0]

    def explore():
        b.policy_explore(0.5, SEED, tick=tick[0])
        tick[0] += 1

    def act():
        b.policy_act(dw.ptr, 0.5, SEED, tick=tick[0], ship_mask_ptr=one)
        tick[0] += 1

    def timed(fn, n):
        b.timer_start()
        for _ in range(n):
            fn()
        return b.timer_stop() / n

    out = {"what": "kernels", "arenas": ARENAS, "ships": M, "block": block, "blocks": blocks}
    b.policy_forward(dw.ptr, one)                            # the handle's results exist
    for name, fn, n in (("explore", explore, block), ("act", act, max(1, block // 5))):
        res = {"A": [], "B": []}
        for i in range(blocks + 2):
            for kind in "AB":
                b.policy_epsilon_ladder(expo if kind == "B" else None)
                ms = timed(fn, n)
                if i >= 2:
                    res[kind].append(ms)
        b.policy_epsilon_ladder(None)
        out[name] = {"calls_per_block": n, "no_ladder": _stats(res["A"]), "ladder": _stats(res["B"]),
                     "ladder_minus_none_us": round(1e3 * float(np.mean(res["B"]) - np.mean(res["A"])), 2)}
    b.restart_random(SEED)
    G = 9
    grp = DeviceBuffer(4 * ARENAS).upload(score_groups(ARENAS, 0, ARENAS, G - 1, EVAL))
    sums = DeviceBuffer(8 * G * (M + 1))
    from ofighters_amd import _native as nat
    grouped = lambda: nat.check(nat.lib().ofx_episode_scores_grouped(b.handle, grp.ptr, G, sums.ptr))
    plain = lambda: b.episode_scores_into(sums.ptr)
    for name, fn in (("scores_grouped_9", grouped), ("scores_plain", plain)):
        ms = [timed(fn, block) for _ in range(blocks + 2)][2:]
        out[name] = _stats(ms)
    b.sync()
    got = sums.download(np.int64, (M + 1,))
    out["check"] = {"plain_count": int(got[-1])}
    b.close()
    return out


def tick():
    repeats, ladder = _arg("--repeats", 5), "--ladder" in sys.argv
    b = ArenaBatch(ARENAS, M)
    eps = Epsilon_decay()
    eps.set(0.1)
    tr = DeviceTrainer(b, synthetic(), epsilon=eps, batch_size=8, memory_size=64, frames=96, fit_batch=256)
    kw = dict(epsilon_ladder=7.0, eval_arenas=EVAL) if ladder else {}
    roll = TrainingRollout(b, tr, ["random"] * M, SEED, policy_ships=(0,), episode_ticks=b.cfg.episode_ticks, **kw)
    roll.run(30)
    b.sync()
    ms, reps = [], []
    for _ in range(repeats):
        n0 = len(roll.losses)
        t0 = time.perf_counter()
        roll.run(120)
        b.sync()
        ms.append((time.perf_counter() - t0) / 120 * 1e3)
        reps.append(len(roll.losses) - n0)
    out = {"what": "tick", "tree": _arg("--tree", "this commit"), "ladder": ladder, "arenas": ARENAS, "ms_per_lock_step": [round(x, 4) for x in ms],
           "replays": reps, "mean_ms": round(float(np.mean(ms)), 4)}
    b.close()
    return out


if __name__ == "__main__":
    what = [x for x in sys.argv[1:] if x in ("kernels", "tick")] or ["kernels", "tick"]
    if "kernels" in what:
        print(json.dumps(kernels()), flush=True)
    if "tick" in what:
        print(json.dumps(tick()), flush=True)
