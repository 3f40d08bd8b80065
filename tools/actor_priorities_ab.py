"""Actor-side initial priorities at the training tick's size (profiles/r13_actor_priorities.txt): `--arenas` (4096)
arenas x 8 ships, one policy ship, memory_size 400, prioritized replay.

cost    One handle, actor priorities enabled, no replays.  Lock-steps of
          A  ofx_policy_forward + ofx_policy_explore + ofx_replay_capture           (the path without the option)
          B  ofx_policy_act + ofx_replay_capture_valued
        each followed by the action packing and the step, alternate in blocks of `--block` (20) lock-steps: `--warmup`
        (50) lock-steps first, then blocks until both have `--steps` (200) timed lock-steps.  A block is timed with
        ofx_timer_* around all of it, so one synchronisation per block.  Reported: ms per lock-step of every block, the
        means, the spread (max - min over blocks) of A, and B - A.  Then the head's streaming kernel alone
        (ofx_policy_profile's event pair) over 20 forwards of each kind: with the probe it runs the instantiation that
        also serves the heat-map output, which is where a difference would come from.
effect  The same configuration as a TrainingRollout with global_sampling=True, `--effect-steps` (600) lock-steps, once
        with the option off and once on: the share of live rows whose mass equals their arena's running maximum.  The
        maximum is read through one more plain capture (its rows enter at mmax[a]).
Usage: python tools/actor_priorities_ab.py [cost] [effect] [--arenas 4096] [--steps 200] [--warmup 50] [--block 20]
                                           [--effect-steps 600]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from ofighters_amd import ArenaBatch, DeviceBuffer
from ofighters_amd.agents.policy_weights import synthetic
from ofighters_amd.lib.epsilon import Epsilon_decay
from ofighters_amd.rollout import TrainingRollout
from ofighters_amd.trainer import DeviceTrainer

M, CAP, SEED, FIT = 8, 400, 0x0F160071, 256


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


ARENAS = _arg("--arenas", 4096)


def cost():
    steps, warmup, block = _arg("--steps", 200), _arg("--warmup", 50), _arg("--block", 20)
    b = ArenaBatch(ARENAS, M)
    b.spawn_random(SEED)
    b.replay_create(CAP, 0)
    b.replay_prioritize(0.6, 1e-3)
    b.replay_actor_priorities(0.9)
    w = synthetic()
    dw = DeviceBuffer(w.nbytes).upload(w)
    mk = np.zeros((ARENAS, M), np.uint8)
    mk[:, 0] = 1
    m_buf = DeviceBuffer(mk.nbytes).upload(mk)               # kept: the pointer alone would outlive its buffer
    m = m_buf.ptr
    b.policy_pin_weights(dw.ptr)
    tick = [0]

    def lockstep(kind):
        t = tick[0]
        b.bot_actions(["random"] * M, SEED, tick=t)
        if kind == "A":
            b.policy_forward(dw.ptr, m)
            b.policy_explore(0.1, SEED, tick=t, ship_mask_ptr=m)
            b.replay_capture(t, ship_mask_ptr=m)
        else:
            b.policy_act(dw.ptr, 0.1, SEED, tick=t, ship_mask_ptr=m)
            b.replay_capture_valued(t, ship_mask_ptr=m)
        b.policy_actions(ship_mask_ptr=m)
        b.step()
        b.rasterise()
        tick[0] += 1
        if tick[0] % 200 == 0:
            b.restart_random(SEED)

    def run_block(kind, n):
        b.timer_start()
        for _ in range(n):
            lockstep(kind)
        return b.timer_stop() / n

    for i in range(warmup):
        lockstep("AB"[i & 1])
    b.sync()
    out = {"what": "cost", "arenas": ARENAS, "warmup": warmup, "block": block, "A_ms": [], "B_ms": []}
    while len(out["A_ms"]) * block < steps:
        out["A_ms"].append(run_block("A", block))
        out["B_ms"].append(run_block("B", block))
    a, bb = np.array(out["A_ms"]), np.array(out["B_ms"])
    out.update(A_mean=float(a.mean()), B_mean=float(bb.mean()), A_spread=float(a.max() - a.min()),
               B_spread=float(bb.max() - bb.min()), B_minus_A=float(bb.mean() - a.mean()))
    for kind in "AB":                                        # the head's streaming kernel alone
        b.sync()
        b.policy_profile(0)
        for _ in range(20):
            lockstep(kind)
        b.sync()
        b.policy_profile(-1)
        out["head_stream_ms_" + kind] = float(np.median([b.event_elapsed(2 * k, 2 * k + 1) for k in range(20)]))
    b.close()
    return out


def effect(actor):
    steps = _arg("--effect-steps", 600)
    b = ArenaBatch(ARENAS, M)
    eps = Epsilon_decay()
    eps.set(0.1)
    tr = DeviceTrainer(b, synthetic(), epsilon=eps, batch_size=8, memory_size=CAP, fit_batch=FIT, seed=SEED,
                       prioritized=True, global_sampling=True, actor_priorities=actor)
    roll = TrainingRollout(b, tr, ["random"] * M, SEED, policy_ships=(0,), episode_ticks=200)
    roll.run(steps)
    b.sync()
    before = [b.replay_priorities(a) for a in range(ARENAS)]
    app0 = b.replay_count()[1]
    b.policy_forward(tr.weights.ptr, roll._mask.ptr)
    b.replay_capture(roll.capture_tick, ship_mask_ptr=roll._mask.ptr)     # plain: the new row's mass is mmax[a]
    b.sync()
    app1 = b.replay_count()[1]
    at_max = live = unread = 0
    for a in range(ARENAS):
        if app1[a] == app0[a]:                                           # the policy ship is latched: mmax[a] not shown
            unread += 1
            continue
        mmax = b.replay_priorities(a)[-1]
        # (a full ring dropped its oldest row for the new one: the rows still live are before[a][1:])
        rows = before[a] if len(before[a]) < CAP else before[a][1:]
        live += len(rows)
        at_max += int((rows == mmax).sum())
    out = {"what": "effect", "actor_priorities": actor, "arenas": ARENAS, "lock_steps": steps, "fits": tr.fit_steps,
           "live_rows": live, "rows_at_mmax": at_max, "share_at_mmax": at_max / max(1, live), "arenas_not_read": unread,
           "distinct_masses": int(len(np.unique(np.concatenate(before))))}
    b.close()
    return out


if __name__ == "__main__":
    what = [x for x in sys.argv[1:] if x in ("cost", "effect")] or ["cost", "effect"]
    if "cost" in what:
        print(json.dumps(cost()), flush=True)
    if "effect" in what:
        for actor in (False, True):
            print(json.dumps(effect(actor)), flush=True)
