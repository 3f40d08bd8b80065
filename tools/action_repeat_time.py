"""Action repeat at the training size (profiles/r17_action_repeat.txt): `--arenas` (4096) arenas x 8 ships, one policy ship.

tick     TrainingRollout + DeviceTrainer (memory 64, frames 96, fit_batch 256, replays on the reference's schedule) with
         action_repeat = `--repeat` K: 32 warm-up lock-steps, then `--repeats` (3) timed runs of `--lock-steps` (480)
         lock-steps each = 480 / K decisions (a host clock around work that ends in a synchronise).  Prints ms per
         decision and ms per lock-step.  With K = 1 it passes nothing the rollout did not have before the option, so the
         same file times a copy of the parent commit: `--root PATH` imports the package from that tree and `--tree NAME`
         labels the line.
kernel   The span kernel alone, from HIP events on the handle's stream (ofx_event_record / ofx_event_elapsed): for K in
         1, 2, 4, 8, alternating blocks of `--block` (20) spans of
           A  one ofx_step_repeat(K), ship 0 of every arena holding an action, span rewards written, no maps
           B  K x (ofx_bot_actions + ofx_step), the two launches per lock-step it replaces
         on two handles in the same state, `--blocks` (8) blocks each after two warm-up blocks; us per span.
Usage: python tools/action_repeat_time.py tick|kernel [--arenas 4096] [--repeat K] [--repeats 3] [--lock-steps 480]
                                          [--block 20] [--blocks 8] [--root PATH] [--tree NAME]

One GPU step per process, each under its own time limit, chained so that a failure ends the chain:
    timeout -k 10 300 python tools/action_repeat_time.py kernel \\
    && timeout -k 10 300 python tools/action_repeat_time.py tick --repeat 1 \\
    && timeout -k 10 300 python tools/action_repeat_time.py tick --repeat 2   (... 4, 8)"""
import json
import os
import sys
import time


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


ROOT = os.path.abspath(_arg("--root", os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)
import numpy as np

from ofighters_amd import ArenaBatch, DeviceBuffer
from ofighters_amd.agents.policy_weights import synthetic
from ofighters_amd.lib.epsilon import Epsilon_decay
from ofighters_amd.rollout import TrainingRollout
from ofighters_amd.trainer import DeviceTrainer

M, SEED = 8, 0x0F160111
ARENAS = _arg("--arenas", 4096)


def tick():
    K, repeats, steps = _arg("--repeat", 1), _arg("--repeats", 3), _arg("--lock-steps", 480)
    if steps % K or 32 % K:
        raise SystemExit("--lock-steps and the 32 warm-up lock-steps must be multiples of --repeat")
    b = ArenaBatch(ARENAS, M)
    eps = Epsilon_decay()
    eps.set(0.1)
    tr = DeviceTrainer(b, synthetic(), epsilon=eps, batch_size=8, memory_size=64, frames=96, fit_batch=256)
    kw = dict(action_repeat=K) if K > 1 else {}
    roll = TrainingRollout(b, tr, ["random"] * M, SEED, policy_ships=(0,), episode_ticks=b.cfg.episode_ticks, **kw)
    roll.run(32 // K)
    b.sync()
    per_decision, per_step, reps = [], [], []
    for _ in range(repeats):
        n0 = len(roll.losses)
        t0 = time.perf_counter()
        roll.run(steps // K)
        b.sync()
        dt = (time.perf_counter() - t0) * 1e3
        per_decision.append(dt / (steps // K))
        per_step.append(dt / steps)
        reps.append(len(roll.losses) - n0)
    out = {"what": "tick", "tree": _arg("--tree", "this commit"), "action_repeat": K, "arenas": ARENAS, "lock_steps": steps,
           "ms_per_decision": [round(x, 4) for x in per_decision], "ms_per_lock_step": [round(x, 4) for x in per_step],
           "replays": reps, "mean_ms_per_decision": round(float(np.mean(per_decision)), 4),
           "mean_ms_per_lock_step": round(float(np.mean(per_step)), 4), "end_tick": int(roll.tick)}
    b.close()
    return out


def kernel():
    block, blocks = _arg("--block", 20), _arg("--blocks", 8)
    beh = ["random"] * M
    mk = np.zeros((ARENAS, M), np.uint8)
    mk[:, 0] = 1
    out = {"what": "kernel", "arenas": ARENAS, "ships": M, "block": block, "blocks": blocks, "spans": {}}
    for K in (1, 2, 4, 8):
        hs = []
        for _ in range(2):                                   # A and B advance alike: the same lasers, the same work
            b = ArenaBatch(ARENAS, M)
            b.spawn_random(SEED)
            b.rollout(beh, SEED, 0, 40)                      # lasers in flight, some ships destroyed
            b.bot_actions(beh, SEED, tick=40)                # ship 0's entry of the action buffer is what A holds
            hs.append(b)
        a, b = hs
        mask = DeviceBuffer(mk.nbytes).upload(mk)
        span = DeviceBuffer(4 * ARENAS * M)
        res = {"A": [], "B": []}
        t = 40
        for i in range(blocks + 2):
            a.event_record(0)
            for j in range(block):
                a.step_repeat(beh, SEED, t + j * K, K, hold_mask_ptr=mask.ptr, span_reward_ptr=span.ptr)
            a.event_record(1)
            b.event_record(0)
            for j in range(block * K):
                b.bot_actions(beh, SEED, tick=t + j)
                b.step()
            b.event_record(1)
            t += block * K
            if i >= 2:
                res["A"].append(a.event_elapsed(0, 1) / block)
                res["B"].append(b.event_elapsed(0, 1) / block)
            a.sync(), b.sync()
        A, B = np.array(res["A"]) * 1e3, np.array(res["B"]) * 1e3
        out["spans"][str(K)] = {"step_repeat_us": [round(float(x), 2) for x in A],
                                "bots_plus_step_us": [round(float(x), 2) for x in B],
                                "step_repeat_mean_us": round(float(A.mean()), 2),
                                "bots_plus_step_mean_us": round(float(B.mean()), 2),
                                "per_lock_step_us": round(float(A.mean()) / K, 2)}
        a.close(), b.close()
    return out


if __name__ == "__main__":
    what = [x for x in sys.argv[1:] if x in ("tick", "kernel")]
    if len(what) != 1:
        raise SystemExit(__doc__)
    print(json.dumps(tick() if what[0] == "tick" else kernel()), flush=True)
