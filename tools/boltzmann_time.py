"""Boltzmann exploration's cost at the training size (profiles/r19_boltzmann.txt): `--arenas` (4096) arenas x 8 ships.

head     One handle, weights pinned, a few lock-steps played.  ofx_policy_profile brackets the streaming head kernel of
         every forward with an event pair, so the figures are the kernel's own time: `--calls` (12) calls each, the first
         two dropped, of
           act        ofx_policy_act at epsilon 0.5            -> k_head_stream<true, 0> (the probe form)
           forward    ofx_policy_forward                       -> k_head_stream<false, 0>
           boltzmann  ofx_policy_act_boltzmann, tau (0.5, 0.5) -> k_head_stream_sample<0>
           boltz_T0   the same at tau (0, 0): the scalar branch skips the noise
         with 1 and with 8 policy ships per arena.
tick     The training tick of bench.py's secondary line (TrainingRollout, one policy ship per arena, memory 64, frames
         96, fit_batch 256, replays on the reference's schedule): 30 warm-up lock-steps, then `--repeats` (5) timed runs
         of 120 lock-steps, ms per lock-step each.  `--boltzmann` turns boltzmann=(0.5, 0.5) on; without it the file uses
         only what the rollout had before the option, so it also times a copy of the parent commit (`--tree NAME`
         labels the line).
near     Exploration quality: `--steps` (600) training lock-steps at 256 arenas under each mode, then the share of the
         rows in the replay memories whose pointer has a marked cell of the row's own ship map within 12 cells
         (Chebyshev): ships are discs of radius 8, so some ship's centre lies within about 20 cells.  A description,
         not a test.
Usage: python tools/boltzmann_time.py [head] [tick] [near] [--arenas 4096] [--calls 12] [--repeats 5] [--boltzmann]
                                      [--tree NAME] [--steps 600]"""
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

M, SEED, TAU = 8, 0x0F160B19, (0.5, 0.5)


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


ARENAS = _arg("--arenas", 4096)


def head():
    calls = _arg("--calls", 12)
    b = ArenaBatch(ARENAS, M)
    b.spawn_random(SEED)
    w = synthetic()
    dw = DeviceBuffer(w.nbytes).upload(w)
    b.policy_pin_weights(dw.ptr)
    for t in range(3):                                       # a few lock-steps: the maps are not the empty start
        b.bot_actions(["random"] * M, SEED, tick=t)
        b.step()
    b.rasterise()
    out = {"what": "head", "arenas": ARENAS, "ships": M, "calls": calls}
    for ships in (1, 8):
        mk = np.zeros((ARENAS, M), np.uint8)
        mk[:, :ships] = 1
        mask = DeviceBuffer(mk.nbytes).upload(mk)
        forms = (("act", lambda t: b.policy_act(dw.ptr, 0.5, SEED, tick=t, ship_mask_ptr=mask.ptr)),
                 ("forward", lambda t: b.policy_forward(dw.ptr, mask.ptr)),
                 ("boltzmann", lambda t: b.policy_act_boltzmann(dw.ptr, 0.5, TAU[0], TAU[1], SEED, tick=t, ship_mask_ptr=mask.ptr)),
                 ("boltz_T0", lambda t: b.policy_act_boltzmann(dw.ptr, 0.5, 0.0, 0.0, SEED, tick=t, ship_mask_ptr=mask.ptr)))
        res = {}
        for name, fn in forms:
            b.sync()
            b.policy_profile(0)
            for t in range(calls):
                fn(t)
            b.sync()
            b.policy_profile(-1)
            ms = [b.event_elapsed(2 * k, 2 * k + 1) for k in range(2, calls)]
            res[name] = {"head_ms": [round(x, 4) for x in ms], "mean_ms": round(float(np.mean(ms)), 4)}
        res["sample_over_forward"] = round(res["boltzmann"]["mean_ms"] / res["forward"]["mean_ms"], 3)
        out["policy_ships_%d" % ships] = res
    b.close()
    return out


def _rollout(arenas, boltzmann, **kw):
    b = ArenaBatch(arenas, M)
    eps = Epsilon_decay()
    eps.set(0.1)
    tr = DeviceTrainer(b, synthetic(), epsilon=eps, batch_size=8, memory_size=64, frames=96, fit_batch=256)
    opt = dict(boltzmann=TAU) if boltzmann else {}
    roll = TrainingRollout(b, tr, ["random"] * M, SEED, policy_ships=(0,), episode_ticks=b.cfg.episode_ticks, **opt, **kw)
    return b, tr, roll


def tick():
    repeats, on = _arg("--repeats", 5), "--boltzmann" in sys.argv
    b, tr, roll = _rollout(ARENAS, on)
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
    out = {"what": "tick", "tree": _arg("--tree", "this commit"), "boltzmann": on, "arenas": ARENAS,
           "ms_per_lock_step": [round(x, 4) for x in ms], "replays": reps, "mean_ms": round(float(np.mean(ms)), 4)}
    b.close()
    return out


def near():
    from ofighters_amd import OfxError
    steps, arenas = _arg("--steps", 600), min(ARENAS, 256)
    out = {"what": "near", "arenas": arenas, "steps": steps, "window": 12}
    for on in (False, True):
        b, tr, roll = _rollout(arenas, on)
        roll.run(steps)
        b.sync()
        hit = total = 0
        for a in range(arenas):
            maps = {}
            for r in b.replay_rows(a):
                t = int(r["tick_prev"])
                if t not in maps:
                    try:
                        maps[t] = b.replay_frame(a, t)[0]       # the ship map the choice was made on, [y][x]
                    except OfxError:
                        maps[t] = None                          # the frame ring no longer holds it
                if maps[t] is None:
                    continue
                px, py = int(r["px"]), int(r["py"])
                hit += bool(maps[t][max(py - 12, 0):py + 13, max(px - 12, 0):px + 13].any())
                total += 1
        out["boltzmann" if on else "epsilon_greedy"] = {"rows": total, "near": hit, "share": round(hit / max(total, 1), 4)}
        b.close()
    return out


if __name__ == "__main__":
    what = [x for x in sys.argv[1:] if x in ("head", "tick", "near")] or ["head", "tick"]
    for name, fn in (("head", head), ("tick", tick), ("near", near)):
        if name in what:
            print(json.dumps(fn()), flush=True)
